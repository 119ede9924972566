// The grouping of a batch's scans into launches (kinematic_icp_amd/csrc/kicp_batch_groups.hpp), driven on the CPU: random batches -
// lengths, group sizes, lane counts, iteration counts per scan, solo scans - through the loop run_batch_groups runs, with the
// "device" replaced by a coin that decides which lane's group completes next.  Checked: every scan is issued exactly once per pass,
// passes in order; never more than G jobs in a launch; a solo scan always alone; scans that go on keep their order in front of the
// fresh ones; fresh scans are taken in batch order; done() counts the finished scans from the front and ends at the batch length.
// Stand-alone (own main), built with -fsanitize=address,undefined by tests/test_batch_groups.py.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "kicp_batch_groups.hpp"

using kicp::host::BatchGroups;

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) {                                                                \
            std::printf("FAILED %s:%d: %s (seed %u)\n", __FILE__, __LINE__, #c, seed); \
            std::exit(1);                                                          \
        }                                                                          \
    } while (0)

struct Lane {
    std::vector<size_t> scans;
    bool active = false, solo = false;
};

static void one_batch(unsigned seed) {
    std::mt19937 rng(seed);
    const size_t count = rng() % 70;
    const int group = 1 + static_cast<int>(rng() % 8), lanes = 1 + static_cast<int>(rng() % 4);
    const unsigned solo_every = rng() % 3 == 0 ? 2 + rng() % 5 : 0;  // (0: no solo scans)
    std::vector<int> need(count), passes(count, 0);
    std::vector<unsigned char> solo(count, 0), finished(count, 0);
    for (size_t k = 0; k < count; ++k) {
        need[k] = rng() % 4 == 0 ? 2 + static_cast<int>(rng() % 9) : 1;  // mostly scans that converge at once
        solo[k] = solo_every && rng() % solo_every == 0;
    }
    BatchGroups sched(count, group, solo);
    std::vector<Lane> L(static_cast<size_t>(lanes));
    std::vector<size_t> carry, out;
    size_t launches = 0, next_fresh = 0, last_done = 0;
    // the launch of a lane's next group, with everything that must hold of it
    auto launch = [&](Lane &g) {
        const bool is_solo = sched.next_group(carry, out);
        CHECK(out.size() <= static_cast<size_t>(group));
        if (out.empty()) {
            CHECK(carry.empty() && sched.issued() == count);
            g.active = false, g.scans.clear();
            return;
        }
        ++launches;
        CHECK(out.size() >= carry.size());
        for (size_t i = 0; i < carry.size(); ++i) CHECK(out[i] == carry[i]);  // what goes on stays in front, in its order
        for (size_t i = carry.size(); i < out.size(); ++i) {                  // then fresh scans in batch order
            CHECK(out[i] == next_fresh && passes[out[i]] == 0);
            ++next_fresh;
        }
        CHECK(sched.issued() == next_fresh);
        for (size_t k : out) {
            CHECK(k < count && !finished[k]);
            CHECK(is_solo == (solo[k] != 0));
            for (const Lane &o : L)  // a scan has one pass out at a time
                if (&o != &g && o.active)
                    for (size_t q : o.scans) CHECK(q != k);
            ++passes[k];
            CHECK(passes[k] <= need[k]);
        }
        if (is_solo) CHECK(out.size() == 1);
        if (out.size() < static_cast<size_t>(group) && !is_solo)  // a group that is not full: nothing was left that could have joined
            CHECK(next_fresh == count || solo[next_fresh]);
        g.scans = out, g.active = true, g.solo = is_solo;
    };
    size_t turns = 0;
    while (!sched.all_finished()) {
        CHECK(++turns < 100000);
        bool any = false;
        for (Lane &g : L) {
            if (!g.active) {
                carry.clear();
                launch(g);
                any = any || g.active;
                continue;
            }
            any = true;
            if (rng() % 3 == 0) continue;  // its rows are not in yet
            carry.clear();
            for (size_t k : g.scans) {
                if (passes[k] < need[k]) {
                    carry.push_back(k);
                } else {
                    finished[k] = 1;
                    sched.finish(k);
                }
            }
            const size_t d = sched.done();
            CHECK(d >= last_done && d <= count);
            for (size_t k = 0; k < d; ++k) CHECK(finished[k]);
            CHECK(d == count || !finished[d]);
            last_done = d;
            launch(g);
        }
        CHECK(any || sched.all_finished());
    }
    CHECK(sched.done() == count && next_fresh == count);
    size_t total = 0;
    for (size_t k = 0; k < count; ++k) {
        CHECK(passes[k] == need[k] && finished[k]);
        total += static_cast<size_t>(need[k]);
    }
    CHECK(launches <= total && (count == 0 || launches >= (total + group - 1) / static_cast<size_t>(group)));
    if (count) sched.finish(0);  // (finishing a scan twice changes nothing)
    CHECK(sched.done() == count);
}

int main() {
    for (unsigned seed = 1; seed <= 3000; ++seed) one_batch(seed);
    std::printf("OK\n");
    return 0;
}
