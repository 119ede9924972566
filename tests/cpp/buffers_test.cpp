// The owning buffer types of kinematic_icp_amd/csrc/kicp_internal.hpp (DevBuf, PinnedBuf, HostStage) on a machine WITHOUT a GPU:
// every allocation fails there, which is the path under test - a failed reserve must leave the buffer empty, whatever it held.
// Built as a stand-alone program together with kicp_core.hip, host code under ASan + UBSan (tests/test_buffers.py).
// A "full" buffer is faked: a sentinel pointer installed through the types' test-only friend, and a free function that only
// records what it is given, so that nothing bogus reaches hipFree / hipHostFree.
#include <cstdio>
#include <utility>

#include "kicp_internal.hpp"

namespace kicp {
namespace host {
struct BufTestAccess {
    template <class T>
    static void fill(DevBuf<T> &b, T *p, size_t cap) { b.p_ = p, b.cap_ = cap; }
    template <class T>
    static void fill(PinnedBuf<T> &b, T *p, size_t cap) { b.p_ = p, b.dev_ = p, b.cap_ = cap; }
};
}  // namespace host
}  // namespace kicp

using namespace kicp::host;

namespace {
int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) ++g_failed, std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
    } while (0)

int g_frees = 0;
void *g_last_freed = nullptr;
hipError_t record_free(void *p) {
    ++g_frees, g_last_freed = p;
    return hipSuccess;
}

template <class B>
bool empty(const B &b) { return b.get() == nullptr && b.capacity() == 0; }
template <class B, class T>
bool holds(const B &b, T *p, size_t cap) { return b.get() == p && b.capacity() == cap; }

// `reserve`: the buffer's growth with the type's own extra arguments bound
template <class B, class T, class Reserve>
void check_buffer(Reserve reserve) {
    static T cells[4];  // sentinels: never dereferenced, never freed
    B::free_fn = record_free;
    {  // empty buffer: nothing to do, nothing to free
        B b;
        CHECK(empty(b));
        CHECK(reserve(b, 0) == KICP_OK && empty(b));
        b.release(), b.release();
        CHECK(empty(b) && g_frees == 0);
    }
    {  // a failed growth of an empty buffer
        B b;
        kicp::host::last_error().clear();
        CHECK(reserve(b, 100) == KICP_ERR_HIP);
        CHECK(empty(b));
        CHECK(kicp_last_error()[0] != '\0');
        CHECK(g_frees == 0);
    }
    {  // ... and of a full one: released first, empty afterwards; a request that fits changes nothing
        B b;
        BufTestAccess::fill(b, &cells[0], 8);
        CHECK(reserve(b, 8) == KICP_OK && reserve(b, 3) == KICP_OK && holds(b, &cells[0], 8) && g_frees == 0);
        kicp::host::last_error().clear();
        CHECK(reserve(b, 9) == KICP_ERR_HIP);
        CHECK(empty(b));
        CHECK(kicp_last_error()[0] != '\0');
        CHECK(g_frees == 1 && g_last_freed == &cells[0]);
        b.release();
        CHECK(g_frees == 1);
    }
    g_frees = 0;
    {  // moves and swap carry pointer and capacity and leave the source empty
        B a;
        BufTestAccess::fill(a, &cells[1], 5);
        B b(std::move(a));
        CHECK(empty(a) && holds(b, &cells[1], 5));
        B c;
        BufTestAccess::fill(c, &cells[2], 7);
        c = std::move(b);  // (what c held is released)
        CHECK(empty(b) && holds(c, &cells[1], 5) && g_frees == 1 && g_last_freed == &cells[2]);
        B &self = c;
        c = std::move(self);
        CHECK(holds(c, &cells[1], 5) && g_frees == 1);
        B d;
        std::swap(c, d);
        CHECK(empty(c) && holds(d, &cells[1], 5) && g_frees == 1);
        d.release();
        CHECK(empty(d) && g_frees == 2 && g_last_freed == &cells[1]);
        d.release();
        CHECK(g_frees == 2);
    }  // (destructors of empty buffers free nothing)
    CHECK(g_frees == 2);
    g_frees = 0;
}

void check_stage() {
    static unsigned char cells[4];
    PinnedBuf<unsigned char>::free_fn = record_free;
    {
        HostStage hs;
        kicp::host::last_error().clear();
        CHECK(stage_reserve(hs, 0, nullptr) == KICP_OK && empty(hs.buf));
        CHECK(stage_reserve(hs, 100, nullptr) == KICP_ERR_HIP);
        CHECK(empty(hs.buf) && hs.buf.dev() == nullptr);
        CHECK(kicp_last_error()[0] != '\0');
        hs.release(), hs.release();
        CHECK(g_frees == 0);
    }
    {  // Full before.  Without a device stage_reserve fails at its stream synchronisation, before anything is let go: the buffer
       // is kept whole then (or, should the synchronisation pass, released and found empty) ...
        HostStage hs;
        BufTestAccess::fill(hs.buf, &cells[0], 8);
        CHECK(stage_reserve(hs, 8, nullptr) == KICP_OK && holds(hs.buf, &cells[0], 8));
        CHECK(stage_reserve(hs, 9, nullptr) == KICP_ERR_HIP);
        CHECK(empty(hs.buf) ? (g_frees == 1 && hs.buf.dev() == nullptr) : (holds(hs.buf, &cells[0], 8) && g_frees == 0));
        hs.release();
        CHECK(empty(hs.buf) && hs.buf.dev() == nullptr && g_frees == 1 && g_last_freed == &cells[0]);
    }
    g_frees = 0;
    {  // ... so its two steps behind that synchronisation are taken here by hand: release, then the failing allocation
        HostStage hs;
        BufTestAccess::fill(hs.buf, &cells[3], 8);
        hs.pending = true;
        hs.release();
        CHECK(empty(hs.buf) && !hs.pending && g_frees == 1 && g_last_freed == &cells[3]);
        kicp::host::last_error().clear();
        CHECK(hs.buf.reserve(9 + 9 / 2 + (1u << 20), hipHostMallocDefault, false) == KICP_ERR_HIP);
        CHECK(empty(hs.buf) && hs.buf.dev() == nullptr && kicp_last_error()[0] != '\0' && g_frees == 1);
    }
    g_frees = 0;
    {  // move-only owner: buffer, event and the pending mark travel together
        HostStage a;
        BufTestAccess::fill(a.buf, &cells[1], 5);
        a.pending = true;
        HostStage b(std::move(a));
        CHECK(empty(a.buf) && !a.pending && a.done == nullptr && holds(b.buf, &cells[1], 5) && b.buf.dev() == &cells[1] && b.pending);
        HostStage c;
        BufTestAccess::fill(c.buf, &cells[2], 7);
        c = std::move(b);
        CHECK(empty(b.buf) && !b.pending && holds(c.buf, &cells[1], 5) && c.pending && g_frees == 1 && g_last_freed == &cells[2]);
        HostStage &self = c;
        c = std::move(self);
        CHECK(holds(c.buf, &cells[1], 5) && c.pending && g_frees == 1);
        HostStage d;
        std::swap(c, d);
        CHECK(empty(c.buf) && !c.pending && holds(d.buf, &cells[1], 5) && d.pending && g_frees == 1);
    }  // (d's destructor releases)
    CHECK(g_frees == 2 && g_last_freed == &cells[1]);
    g_frees = 0;
}
}  // namespace

int main() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
        std::printf("skipped: a device is present, allocations would succeed\n");
        return 0;
    }
    static_assert(!std::is_copy_constructible<DevBuf<double>>::value && !std::is_copy_assignable<DevBuf<double>>::value, "DevBuf is move-only");
    static_assert(!std::is_copy_constructible<PinnedBuf<double>>::value && !std::is_copy_assignable<PinnedBuf<double>>::value, "PinnedBuf is move-only");
    static_assert(!std::is_copy_constructible<HostStage>::value && !std::is_copy_assignable<HostStage>::value, "HostStage is move-only");
    static_assert(!std::is_convertible<DevBuf<double>, double *>::value && !std::is_convertible<PinnedBuf<double>, double *>::value, "no implicit conversion to T *");
    check_buffer<DevBuf<double>, double>([](DevBuf<double> &b, size_t n) { return b.reserve(n); });
    check_buffer<PinnedBuf<uint32_t>, uint32_t>([](PinnedBuf<uint32_t> &b, size_t n) { return b.reserve(n, hipHostMallocMapped | hipHostMallocCoherent); });
    check_buffer<PinnedBuf<unsigned char>, unsigned char>([](PinnedBuf<unsigned char> &b, size_t n) { return b.reserve(n, hipHostMallocDefault, false); });
    check_stage();
    if (g_failed) return 1;
    std::printf("ok %d\n", g_checks);
    return 0;
}
