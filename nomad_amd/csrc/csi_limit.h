// LimitIterator + MaxScoreIterator (scheduler/select.go:35-67, :95-116) over a
// source that may return a nil which is not the end of the stream: the nil
// FeasibilityWrapper.Next returns at an unavailable node of a class already
// memoised eligible (feasible.go:1112-1119). The rank iterators between the
// two pass a nil up unchanged, and the next call of the source goes on with
// the following node.
//
// The fold is written once, as a state machine stepped with one source event
// at a time: k_csi_loop steps it on the device, pe_csi_limit_fold on the host
// (the tests' entry), and both run these lines.
//
// LimitIterator.Next calls source.Next() at three places; the phase says which
// one the next event answers:
//   kCsiTop   nextOption at the top of Next (select.go:39)
//   kCsiSkip  the skip loop (:48)
//   kCsiAfter nextOption after the skip loop (:53)
// A nil at kCsiTop or kCsiAfter pops a skipped option if one is pending, else
// the Select ends. A popped option at kCsiTop runs the threshold test again:
// with fewer than maxSkip entries it is appended a second time (a duplicate
// entry) and the skip loop pulls the source again, so the walk resumes past
// the stop. A nil in the skip loop ends the loop, counts the Next (`seen`) and
// pulls again at kCsiAfter, whose option is returned without the threshold
// test. MaxScoreIterator keeps the first strict maximum in return order
// (select.go:107); the events arrive in that order, so a plain `>` is the rule.
//
// Bound: every event either consumes one source position, pops one skipped
// entry (at most kCsiMaxSkip appends, so at most kCsiMaxSkip pops), moves
// kCsiSkip -> kCsiAfter (once per append run, at most kCsiMaxSkip times) or
// ends the Select. After the source's last position a caller feeds at most
// kCsiTailEvents nils.
#pragma once
#include <stdint.h>

#if defined(__HIP__)   // compiled as HIP (kernels.hip); plain C++ elsewhere
#define PE_CSI_HD __host__ __device__ __forceinline__
#else
#define PE_CSI_HD inline
#endif

namespace pe {

constexpr int kCsiMaxSkip = 3;          // LimitIterator.maxSkip (stack.go: SetLimit's maxSkip = 3)
constexpr int kCsiTailEvents = 2 * kCsiMaxSkip + 2;
enum : uint32_t { kCsiTop = 0, kCsiSkip = 1, kCsiAfter = 2 };
enum : uint32_t { kCsiOption = 0, kCsiNil = 1 };

struct CsiLimit {
    uint32_t limit, seen;
    uint32_t n_skip, pop;               // skippedNodes' length, skippedNodeIndex
    uint32_t phase;
    uint32_t ended_nil;                 // the Select ended at a nil Next (not at seen == limit)
    int32_t best_id;                    // -1: no option returned yet
    double best_score;
    double skip_score[kCsiMaxSkip];
    int32_t skip_id[kCsiMaxSkip];
};

// Returns true when the Select is over before any source event (limit 0).
PE_CSI_HD bool csi_limit_init(CsiLimit& L, uint32_t limit) {
    L.limit = limit;
    L.seen = 0;
    L.n_skip = 0;
    L.pop = 0;
    L.phase = kCsiTop;
    L.ended_nil = 0;
    L.best_id = -1;
    L.best_score = 0.0;
    for (int i = 0; i < kCsiMaxSkip; i++) { L.skip_score[i] = 0.0; L.skip_id[i] = -1; }
    return limit == 0;
}

// One source event: an option (score, id) or a nil. `threshold` is
// LimitIterator.scoreThreshold (0.0 on every stack). Returns true when the
// Select is over: MaxScoreIterator got a nil Next, or the next Next would find
// seen == limit (which pulls nothing from the source).
PE_CSI_HD bool csi_limit_step(CsiLimit& L, uint32_t kind, double score, int32_t id, double threshold = 0.0) {
    bool test = true;                   // the option still faces the threshold test
    if (kind == kCsiNil) {
        if (L.phase == kCsiSkip) {      // select.go:48 -> the loop ends; :52 seen++; :53 pulls again
            L.seen++;
            L.phase = kCsiAfter;
            return false;
        }
        if (L.pop >= L.n_skip) {        // nextOption has nothing pending: Next returns nil
            L.ended_nil = 1;
            return true;
        }
        for (int i = 0; i < kCsiMaxSkip; i++)   // select.go:61-64 (no dynamic index: the arrays stay in registers)
            if ((uint32_t)i == L.pop) { score = L.skip_score[i]; id = L.skip_id[i]; }
        L.pop++;
    }
    if (L.phase == kCsiAfter) test = false;
    if (test && L.n_skip < (uint32_t)kCsiMaxSkip && score <= threshold) {
        // select.go:44-49: set aside (a popped option a second time), pull again
        for (int i = 0; i < kCsiMaxSkip; i++)
            if ((uint32_t)i == L.n_skip) { L.skip_score[i] = score; L.skip_id[i] = id; }
        L.n_skip++;
        L.phase = kCsiSkip;
        return false;
    }
    if (L.phase != kCsiAfter) L.seen++;   // (kCsiAfter: counted when the skip loop ended)
    // MaxScoreIterator.Next (select.go:103-109)
    if (L.best_id < 0 || score > L.best_score) { L.best_score = score; L.best_id = id; }
    L.phase = kCsiTop;
    return L.seen == L.limit;
}

}  // namespace pe
