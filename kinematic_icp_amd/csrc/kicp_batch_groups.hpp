// kicp_batch_groups.hpp -- which scans of a batch share a launch (run_batch_groups, kicp_reg_queues.hip).  Bookkeeping only: no HIP,
// no handle, nothing of the device in here, so that tests/cpp/batch_groups_test.cpp can drive it on the CPU with made-up
// convergence patterns.
//
// A batch is `count` independent scans, taken in order.  A LANE (a queue with a host loop behind it) launches GROUPS of up to
// `group` jobs; a job is the next pass of one scan.  When all rows of a group are in, the lane tells the scheduler which of its
// scans go on (next_group's `carry`) and which are finished (finish), and gets its next group: the scans that go on, in the order
// they had, then fresh scans from the front of what is left, up to `group`.  A scan marked SOLO (one that takes a kernel of its own:
// the small-scan kernels, sub-lanes per query) never shares a launch: it is a group of one from its first pass to its last.
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace kicp {
namespace host {

class BatchGroups {
public:
    BatchGroups(size_t count, int group, std::vector<unsigned char> solo = {})
        : count_(count), group_(group < 1 ? 1 : static_cast<size_t>(group)), solo_(std::move(solo)), complete_(count, 0) {
        solo_.resize(count, 0);
    }
    // The lane's next group into `out` (empty: nothing left for this lane).  `carry`: the scans of the group it has just collected
    // that need another pass.  Returns true when the group is a solo scan's.
    bool next_group(const std::vector<size_t> &carry, std::vector<size_t> &out) {
        out.clear();
        for (size_t k : carry) out.push_back(k);
        if (!out.empty() && solo_[out[0]]) return true;  // (a solo scan came alone and goes on alone)
        while (out.size() < group_ && next_ < count_) {
            if (solo_[next_]) {
                if (out.empty()) {
                    out.push_back(next_++);
                    return true;
                }
                break;  // it waits for a launch of its own: the scans are taken in order
            }
            out.push_back(next_++);
        }
        return false;
    }
    void finish(size_t k) {
        if (!complete_[k]) complete_[k] = 1, ++finished_;
    }
    bool all_finished() const { return finished_ == count_; }
    size_t issued() const { return next_; }  // scans that have had their first pass launched
    // scans completed from the front: what a call that ends early may report as done
    size_t done() {
        while (front_ < count_ && complete_[front_]) ++front_;
        return front_;
    }

private:
    size_t count_, group_;
    std::vector<unsigned char> solo_, complete_;
    size_t next_ = 0, front_ = 0, finished_ = 0;
};

}  // namespace host
}  // namespace kicp
