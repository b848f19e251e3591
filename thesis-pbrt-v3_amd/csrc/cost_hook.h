// hprt — the costing hook of the tree builders (rbsp_builder.cpp, bsppaper_builder.cpp, bspnode_builder.cpp): a node's split
// candidates costed elsewhere (the device-assisted builds, hprt_*_build*_device) and the ones flagged uncosted repaired by the
// builder's own code.  The contract is stated once in DESIGN.md 8p.  Host code only.
#pragma once
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

namespace hprt {

struct BuildDeviceStats { uint64_t nodesDevice = 0, candidatesDevice = 0, candidatesRecosted = 0, nodesHost = 0; double secondsDevice = 0; };

// What a builder's params carry for the hook; Request is the builder's view of one node's candidates (its costs, costsFixed and
// overflow arrays among them).  A node with at least costMinCandidates candidates is handed to costFn instead of the thread
// pool.  costFn fills costs / costsFixed / overflow for every candidate and returns 0; 1 declines the node (it takes the host
// path); < 0 fails the build with *err.  Smaller nodes, and all nodes when costFn is empty, take the host path.  The scan over
// costs[] is the same either way.
template <class Request>
struct CostHook {
    std::function<int(const Request &, std::string *err)> costFn;
    uint32_t costMinCandidates = 1024;    // (kdop::kParallelCandidates)
    BuildDeviceStats *stats = nullptr;    // filled when costFn is set
    // Diagnostics: called for a node costFn has handled, after the repair, with the costs (and counts) the scan is about to read
    std::function<void(const Request &)> costDone;
};

enum class HookResult { NotCosted, Costed, Failed };

// One node of n candidates.  fill(rq) fills the request (overflow, n zeroed flags, is the array to point rq.overflow at) and runs
// only when the hook is engaged; repair(k) costs candidate k with the builder's own code.  Costed: costs[] is complete.
// NotCosted: the caller costs the node (counted in stats->nodesHost).  Failed: *err says why.  timeRepair: secondsDevice spans
// costFn and the repair; else costFn alone.
template <class Request, class Fill, class Repair>
HookResult RunCostHook(const CostHook<Request> &h, size_t n, std::vector<uint8_t> &overflow, bool timeRepair, Fill fill, Repair repair, std::string *err) {
    using Clock = std::chrono::steady_clock;
    if (h.costFn && n >= 1 && n >= h.costMinCandidates) {
        overflow.assign(n, 0);
        Request rq;
        fill(rq);
        const auto t0 = Clock::now();
        const int rc = h.costFn(rq, err);
        auto t1 = Clock::now();
        if (rc < 0) {
            if (err->empty()) *err = "the costing hook failed";
            return HookResult::Failed;
        }
        if (rc == 0) {
            uint64_t redo = 0;
            for (size_t k = 0; k < n; ++k)
                if (overflow[k]) { repair(k); ++redo; }
            if (h.stats) {
                if (timeRepair) t1 = Clock::now();
                h.stats->secondsDevice += std::chrono::duration<double>(t1 - t0).count();
                ++h.stats->nodesDevice; h.stats->candidatesDevice += n - redo; h.stats->candidatesRecosted += redo;
            }
            if (h.costDone) h.costDone(rq);
            return HookResult::Costed;
        }
    }
    if (h.stats) ++h.stats->nodesHost;
    return HookResult::NotCosted;
}

}  // namespace hprt
