// LimitIterator + MaxScoreIterator (scheduler/select.go:35-67, :95-116) over a
// source that may return a nil which is not the end of the stream: the nil
// FeasibilityWrapper.Next returns at an unavailable node of a class already
// memoised eligible (feasible.go:1112-1119). The rank iterators between the
// two pass a nil up unchanged, and the next call of the source goes on with
// the following node.
//
// The fold is written once, as a state machine stepped with one source event
// at a time: k_csi_loop steps it on the device, pe_csi_limit_fold on the host
// (the tests' entry), and both run these lines. At limit MaxInt32 runs of
// options collapse into one event each (below: csi_limit_run, csi_full_fold),
// which k_csi_full and pe_csi_full_fold run.
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

// ---- the fold at an unbounded limit (k_csi_full, pe_csi_full_fold) --------------------
// At limit MaxInt32 (stack.go:165-167) `seen == limit` never fires, and two
// facts of csi_limit_step make the event stream compressible: an option with
// score > threshold is returned in every phase, and once n_skip == kCsiMaxSkip
// every option is returned. A maximal run of consecutive such options (no nil
// inside) therefore equals one option event that carries the run's first
// strict maximum and its id: phase, n_skip, pop, best_* and ended_nil come out
// identical, and `seen` grows by the run's length, minus one when the run
// starts in kCsiAfter (that Next was counted when the skip loop ended).
//
// What is still stepped one at a time (the specials): nils, and non-positive
// options that arrive while n_skip < kCsiMaxSkip. Such an option is either
// appended (at most kCsiMaxSkip appends, duplicates included) or returned at
// kCsiAfter (once per append run), so there are at most kCsiFullOptions of
// them per Select, and they are the first non-positive options of the stream.
// A nil moves kCsiSkip -> kCsiAfter (once per append run), pops an entry (at
// most kCsiMaxSkip) or ends the Select: at most kCsiFullNils per Select, so no
// position past the kCsiFullNils-th nil is ever consumed.
constexpr uint32_t kCsiUnbounded = 0x7FFFFFFFu;
constexpr int kCsiFullOptions = 2 * kCsiMaxSkip;
constexpr int kCsiFullNils = 2 * kCsiMaxSkip + 1;
constexpr int kCsiFullSpecials = kCsiFullOptions + kCsiFullNils;

// `count` consecutive options, each of which csi_limit_step would return
// (score > threshold, or n_skip == kCsiMaxSkip), as one event: (score, id) is
// the run's first strict maximum. For a fold at limit kCsiUnbounded only.
PE_CSI_HD void csi_limit_run(CsiLimit& L, uint32_t count, double score, int32_t id) {
    if (count == 0) return;
    L.seen += count - (L.phase == kCsiAfter ? 1u : 0u);
    if (L.best_id < 0 || score > L.best_score) { L.best_score = score; L.best_id = id; }
    L.phase = kCsiTop;
}

struct CsiSpecial {     // an event stepped on its own, at source position `pos`
    uint32_t pos, kind; // kCsiNil, or kCsiOption with a score <= threshold
    double score;
};
struct CsiSegment {     // the positions between two specials, collapsed
    uint32_t options;   // options among them
    uint32_t nonpos;    // of which score <= threshold
    int32_t id;         // first strict maximum over the options
    uint32_t _pad;
    double score;
};

// One Select at limit kCsiUnbounded over specials in position order and the
// collapsed segments around them: seg[i] precedes sp[i], seg[n_spec] follows
// the last special up to the end of the source. `closed`: the source was cut
// after its kCsiFullNils-th nil, which is sp[n_spec - 1] (no seg[n_spec]).
// Returns 0 when the Select ended at special *ended_at, 1 when it ended at the
// nils after the source's last position, -1 when a bound above does not hold
// (a non-positive option inside a segment entered with n_skip < kCsiMaxSkip,
// a closed source that did not end the Select, tail nils that did not).
PE_CSI_HD int csi_full_fold(CsiLimit& L, const CsiSegment* seg, const CsiSpecial* sp, uint32_t n_spec, bool closed,
                            uint32_t* ended_at) {
    csi_limit_init(L, kCsiUnbounded);
    if (n_spec > (uint32_t)kCsiFullSpecials) return -1;
    for (uint32_t i = 0; i <= n_spec; i++) {
        if (i < n_spec || !closed) {
            const CsiSegment g = seg[i];
            if (g.options) {
                if (g.nonpos && L.n_skip < (uint32_t)kCsiMaxSkip) return -1;
                csi_limit_run(L, g.options, g.score, g.id);
            }
        }
        if (i == n_spec) break;
        if (csi_limit_step(L, sp[i].kind, sp[i].score, (int32_t)sp[i].pos)) {
            *ended_at = i;
            return 0;
        }
    }
    if (closed) return -1;
    for (int t = 0; t < kCsiTailEvents; t++)
        if (csi_limit_step(L, kCsiNil, 0.0, -1)) {
            *ended_at = n_spec;
            return 1;
        }
    return -1;
}

// The compression of a plain stream, as k_csi_full's passes do it: the first
// kCsiFullNils nils, the first kCsiFullOptions non-positive options before the
// last of those nils, and per segment between them the option count, the
// non-positive count and the first strict maximum. Item i is an option with
// scores[i] (kind 0) or a nil (kind 1). seg has kCsiFullSpecials + 1 entries,
// sp kCsiFullSpecials. Returns the number of specials; *closed as above.
inline uint32_t csi_full_compress(const double* scores, const uint8_t* kind, uint32_t n, CsiSegment* seg,
                                  CsiSpecial* sp, bool* closed, double threshold = 0.0) {
    uint32_t end = n, nils = 0;
    for (uint32_t i = 0; i < n && nils < (uint32_t)kCsiFullNils; i++)
        if (kind[i] && ++nils == (uint32_t)kCsiFullNils) end = i + 1;
    *closed = nils == (uint32_t)kCsiFullNils;
    uint32_t n_spec = 0, n_np = 0;
    CsiSegment cur = {0, 0, -1, 0, 0.0};
    for (uint32_t i = 0; i < end; i++) {
        const bool np = !kind[i] && scores[i] <= threshold;
        if (kind[i] || (np && n_np < (uint32_t)kCsiFullOptions)) {
            seg[n_spec] = cur;
            cur = CsiSegment{0, 0, -1, 0, 0.0};
            sp[n_spec].pos = i;
            sp[n_spec].kind = kind[i] ? kCsiNil : kCsiOption;
            sp[n_spec].score = kind[i] ? 0.0 : scores[i];
            n_spec++;
            n_np += np ? 1u : 0u;
            continue;
        }
        if (cur.options == 0 || scores[i] > cur.score) { cur.score = scores[i]; cur.id = (int32_t)i; }
        cur.options++;
        cur.nonpos += np ? 1u : 0u;
    }
    seg[n_spec] = cur;
    return n_spec;
}

}  // namespace pe
