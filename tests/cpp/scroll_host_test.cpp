// scroll_host_test.cpp -- kicp_scroll_host.hpp in a program of its own (tests/test_scroll_host.py builds it plainly and under ASan +
// UBSan and compares what it writes with tests/scroll_ref.py): the shift of a plane, the follow rule, the origin rule and the window.
//   in:  uint32 W, H, elem_bytes, n_shifts, n_follow, n_origin, n_window, 0; int32 (dx, dy) x n_shifts; int64 (c, size, margin, step) x
//        n_follow; float64 (origin, d, cell) x n_origin; int32 (win_x0, win_y0, dx, dy) x n_window; the plane, W * H * elem_bytes bytes
//   out: the shifted plane per shift; int64 (ok, d) x n_follow; float64 x n_origin; int32 (kept, win_x0, win_y0) x n_window
// Every buffer is allocated at exactly its size, so a byte too many is a sanitizer report.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kicp_scroll_host.hpp"

using namespace kicp;

template <class T>
static std::vector<T> take(std::FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && std::fread(v.data(), sizeof(T), n, f) != n) std::fprintf(stderr, "short input\n"), std::exit(2);
    return v;
}
template <class T>
static void put(std::FILE *f, const std::vector<T> &v) {
    if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) std::fprintf(stderr, "short output\n"), std::exit(2);
}

int main(int argc, char **argv) {
    if (argc != 3) return std::fprintf(stderr, "usage: %s in out\n", argv[0]), 2;
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) return std::fprintf(stderr, "cannot open the files\n"), 2;
    const std::vector<uint32_t> head = take<uint32_t>(in, 8);
    const uint32_t W = head[0], H = head[1], elem = head[2];
    const std::vector<int32_t> shifts = take<int32_t>(in, 2 * static_cast<size_t>(head[3]));
    const std::vector<int64_t> follow = take<int64_t>(in, 4 * static_cast<size_t>(head[4]));
    const std::vector<double> origin = take<double>(in, 3 * static_cast<size_t>(head[5]));
    const std::vector<int32_t> window = take<int32_t>(in, 4 * static_cast<size_t>(head[6]));
    const size_t bytes = static_cast<size_t>(W) * H * elem;
    const std::vector<unsigned char> plane = take<unsigned char>(in, bytes);
    for (size_t k = 0; k < head[3]; ++k) {
        std::vector<unsigned char> shifted(bytes, 0xA5);
        scroll_host::shift_plane(plane.data(), shifted.data(), W, H, elem, shifts[2 * k], shifts[2 * k + 1]);
        if (scroll_empties(W, H, shifts[2 * k], shifts[2 * k + 1]))
            for (unsigned char b : shifted)
                if (b) return std::fprintf(stderr, "an emptying shift left a byte\n"), 1;
        put(out, shifted);
    }
    std::vector<int64_t> followed;
    for (size_t k = 0; k < head[4]; ++k) {
        long long d = 0;
        const bool ok = scroll_host::follow_shift(follow[4 * k], static_cast<uint32_t>(follow[4 * k + 1]), static_cast<uint32_t>(follow[4 * k + 2]),
                                                  static_cast<uint32_t>(follow[4 * k + 3]), &d);
        followed.push_back(ok ? 1 : 0), followed.push_back(ok ? d : 0);
    }
    put(out, followed);
    std::vector<double> origins;
    for (size_t k = 0; k < head[5]; ++k) origins.push_back(scroll_host::scroll_origin(origin[3 * k], static_cast<int32_t>(origin[3 * k + 1]), origin[3 * k + 2]));
    put(out, origins);
    std::vector<int32_t> windows;
    for (size_t k = 0; k < head[6]; ++k) {
        int32_t x0 = window[4 * k], y0 = window[4 * k + 1];
        const bool kept = scroll_host::scroll_window(x0, y0, window[4 * k + 2], window[4 * k + 3]);
        windows.push_back(kept ? 1 : 0), windows.push_back(x0), windows.push_back(y0);
    }
    put(out, windows);
    std::fclose(in);
    return std::fclose(out) == 0 ? 0 : 2;
}
