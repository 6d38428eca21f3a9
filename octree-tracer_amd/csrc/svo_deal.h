// svo_deal.h -- a resting view's static deal: which wave traces which strips, in which order, written down once
// and replayed without claims (trace_stack_replay_kernel), then improved from per-wave time stamps.  Plain C++ that host and
// device both include, the way svo_rules.h is: svo_deal.hip runs seed, step and compare as kernels of one workgroup (thread
// `tid` of `nt`, `sync` = the workgroup's barrier), tests/deal_driver.cpp runs the same functions as one thread.  The host's
// part (deal_before_trace / deal_after_post) decides per frame what svo_abi.cpp launches; it knows frame counts only -- what
// the steps found stays on the device, and the host sees it through a mirror it never waits for.
#pragma once
#include <cstddef>
#include <cstdint>

#include "svo_sched.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SVO_DEAL_HD __host__ __device__
#else
#define SVO_DEAL_HD
#endif

namespace svo {

// replayed frames of a resting view after which a step moves strips (the seed's own frame is the first of them; the last one
// puts the best table back): a policy constant like kBalanceLearnFrames
constexpr uint32_t kDealLearnFrames = 16;
constexpr uint32_t kDealEnd = 0xFFFFFFFFu;     // behind a row's last entry
constexpr uint32_t kDealMaxRow = 256;          // a frame whose rows would need more entries stays with the claiming kernel
constexpr uint32_t kDealMaxListWaves = 1024;   // ... and so does a grid with more waves on a list (the step ranks them in LDS)
constexpr uint32_t kDealPairsDiv = 16;         // a step pairs the latest 1 / kDealPairsDiv of a list's waves with its earliest
// the balance words the deal reads (svo_device.h has them for the trace kernel; the same numbers, checked there)
constexpr uint32_t kDealBalStart = 9, kDealBalStamps = 19, kDealBalBestTime = 20, kDealBalHead = 32, kDealBalSlots = 4096;

// device state words
enum : uint32_t {
    kDealStep = 0,        // replayed frames stepped since the seed (kDealLearnFrames: learning is over)
    kDealBestTime = 1,    // the shortest replayed frame so far: latest wave end - start stamp, 10 ns ticks
    kDealBestSample = 2,  // that frame measured the way balance_step measures a claimed frame (the sampled workgroup stamps)
    kDealVerdict = 3,     // 0: learning, 1: the view rests on its best table, 2: "claims" -- replay never beat the claiming kernel
    kDealSeeds = 4,       // seeds since the buffers were made
    kDealMoves = 5,       // strips moved since the buffers were made
    kDealLastTime = 6,    // the last stepped frame's time
    kDealLastMoves = 7,   // ... and moves
    kDealClaimTime = 8,   // the last frame the claiming kernel traced from the seeded lists, measured like kDealBestSample
    kDealBestStep = 9,    // the stepped frame (0: the seed's own) whose table is the best so far
    kDealTmpTime = 16,    // between a step's two kernels: the stepped frame's time, its sampled time, and (8 words) every list's moves
    kDealTmpSample = 17,
    kDealTmpMoves = 18,
    kDealStateWords = 32
};

struct Deal {
    uint32_t *table;         // rows of row_cap entries, one per wave of the grid
    uint32_t *len;           // the rows' lengths (the steps keep them; the replay kernel reads the terminators)
    uint32_t *log;           // the moves of every step, (donor, receiver) in fixed slots (deal_log_slot): undone, last first, they give
                             // back the table any earlier frame was traced with -- that is how the best table is kept
    uint32_t *lists;         // the lists the table was seeded from: 8 lengths, then 8 lists of order_cap entries
    uint32_t *stamps;        // per wave: when it began to generate its last strip, when it ended
    uint32_t *state;         // kDealStateWords
    uint32_t row_cap, grid_blocks, order_cap, pairs_div;
};

// The grid is the trace kernel's: workgroup b starts on list b % 8, four waves each; rank r among the waves of list l.
SVO_DEAL_HD inline uint32_t deal_list_waves(uint32_t grid_blocks, uint32_t l) { return ((grid_blocks + 7u - l) / 8u) * 4u; }
SVO_DEAL_HD inline uint32_t deal_wave(uint32_t l, uint32_t rank) { return ((rank >> 2) * 8u + l) * 4u + (rank & 3u); }
// slot of pair p of list l in step s of the move log: a step has at most half of a list's waves as pairs
SVO_DEAL_HD inline uint32_t deal_log_slot(uint32_t grid_blocks, uint32_t s, uint32_t l, uint32_t p) {
    uint32_t before = 0u;
    for (uint32_t k = 0; k < l; k++) before += deal_list_waves(grid_blocks, k) / 2u;
    return s * (grid_blocks * 2u) + before + p;
}
inline size_t deal_log_words(uint32_t grid_blocks) { return (size_t)kDealLearnFrames * grid_blocks * 2u * 2u; }

// Entries a row gets: at least twice the longest row a seed can make (a list holds at most order_cap strips), a power of two.
// 0: this frame stays with the claiming kernel (rows too long, a list without waves, too many waves to rank).
inline uint32_t deal_row_cap(uint32_t order_cap, uint32_t grid_blocks) {
    if (grid_blocks < 8u || deal_list_waves(grid_blocks, 0u) > kDealMaxListWaves) return 0u;
    const uint32_t w_min = deal_list_waves(grid_blocks, 7u);
    const uint32_t longest = (order_cap + w_min - 1u) / w_min;
    uint32_t cap = 2u;
    while (cap < 2u * longest + 1u) cap *= 2u;  // (+ 1: the terminator)
    return cap <= kDealMaxRow ? cap : 0u;
}

// (as balance_step: a stamp that was never written, a difference that wrapped)
SVO_DEAL_HD inline bool deal_valid_time(uint32_t t) { return t != 0u && t < 100000000u; }

// the largest of the threads' values; red: nt words of the workgroup's
template <typename Sync>
SVO_DEAL_HD inline uint32_t deal_reduce_max(uint32_t *red, uint32_t mine, uint32_t tid, uint32_t nt, Sync sync) {
    red[tid] = mine;
    sync();
    if (tid == 0u) {
        uint32_t m = 0u;
        for (uint32_t i = 0; i < nt; i++) m = red[i] > m ? red[i] : m;
        red[0] = m;
    }
    sync();
    const uint32_t m = red[0];
    sync();
    return m;
}

// A frame's time the way balance_step measures it: the latest of the sampled workgroup stamps behind the balance words.
template <typename Sync>
SVO_DEAL_HD inline uint32_t deal_sample_time(const uint32_t *bal, uint32_t *red, uint32_t tid, uint32_t nt, Sync sync) {
    const uint32_t t0 = bal[kDealBalStart], n_slots = bal[kDealBalStamps] < kDealBalSlots ? bal[kDealBalStamps] : kDealBalSlots;
    uint32_t mine = 0u;
    for (uint32_t i = tid; i < n_slots; i += nt) {
        const uint32_t t = bal[kDealBalHead + i] - t0;
        if (deal_valid_time(t) && t > mine) mine = t;
    }
    return deal_reduce_max(red, mine, tid, nt, sync);
}

// Seed: entry k of list l goes to wave k mod W_l of that list, at position k div W_l -- the stratified deal the run-ahead claims
// make in the ideal case.  Keeps a copy of the lists and starts learning over.  bal (or null): the balance words of the frame
// before, which the claiming kernel traced from these lists -- its time is what replay has to beat (red: nt words).
template <typename Sync>
SVO_DEAL_HD inline void deal_seed(const Deal &d, const uint32_t *order, const uint32_t *bal, uint32_t *red, uint32_t tid, uint32_t nt, Sync sync) {
    const uint32_t t_claims = bal ? deal_sample_time(bal, red, tid, nt, sync) : 0u;
    for (uint32_t i = tid; i < 8u + 8u * d.order_cap; i += nt) d.lists[i] = order[i];
    for (uint32_t l = 0; l < 8u; l++) {
        const uint32_t w = deal_list_waves(d.grid_blocks, l);
        const uint32_t len = order[l] < d.order_cap ? order[l] : d.order_cap;
        for (uint32_t k = tid; k < len; k += nt) d.table[deal_wave(l, k % w) * d.row_cap + k / w] = order[8u + l * d.order_cap + k];
        for (uint32_t r = tid; r < w; r += nt) {  // the terminator behind the row's last entry (what lies behind it is never read)
            const uint32_t n = len > r ? (len - r + w - 1u) / w : 0u;
            d.table[deal_wave(l, r) * d.row_cap + n] = kDealEnd;
            d.len[deal_wave(l, r)] = n;
        }
    }
    if (tid == 0u) {
        d.state[kDealStep] = 0u;
        d.state[kDealBestTime] = d.state[kDealBestSample] = 0u;
        d.state[kDealVerdict] = 0u;
        d.state[kDealBestStep] = 0u;
        d.state[kDealSeeds] += 1u;
        if (bal) d.state[kDealClaimTime] = t_claims;
    }
    sync();
}

// After the lists were rebuilt from the same input (the schedule's 64-frame backstop): the table stays when they are the lists
// it was seeded from; else it is seeded again.  flag: one word of the workgroup's.
template <typename Sync>
SVO_DEAL_HD inline void deal_reseed_if_changed(const Deal &d, const uint32_t *order, uint32_t *flag, uint32_t tid, uint32_t nt, Sync sync) {
    if (tid == 0u) *flag = 0u;
    sync();
    bool differs = false;
    for (uint32_t l = tid; l < 8u; l += nt) differs = differs || d.lists[l] != order[l];
    for (uint32_t i = tid; i < 8u * d.order_cap; i += nt) {
        const uint32_t l = i / d.order_cap, k = i - l * d.order_cap;
        if (k < d.lists[l] && k < order[l]) differs = differs || d.lists[8u + i] != order[8u + i];
    }
    if (differs) *flag = 1u;
    sync();
    const bool reseed = *flag != 0u;
    sync();
    if (reseed) deal_seed(d, order, nullptr, nullptr, tid, nt, sync);  // (the frame before was a replayed one: the claims' time stays)
}

// Move the donor's last strip to the end of the receiver's row, if the move can pay for itself: the donor ended later than the
// receiver by more than its last strip took (end - begin of that strip), keeps a strip, and the receiver has room.  Rows stay
// longest-first: a row's last strip is its cheapest and is appended last.
SVO_DEAL_HD inline void deal_move_last(const Deal &d, uint32_t from, uint32_t to) {
    uint32_t *const rf = d.table + from * d.row_cap, *const rt = d.table + to * d.row_cap;
    const uint32_t nf = d.len[from] - 1u, nt = d.len[to];
    rt[nt] = rf[nf];
    rt[nt + 1u] = kDealEnd;
    rf[nf] = kDealEnd;
    d.len[from] = nf;
    d.len[to] = nt + 1u;
}
SVO_DEAL_HD inline bool deal_try_move(const Deal &d, uint32_t donor, uint32_t receiver, uint32_t t0, uint32_t slot) {
    const int32_t end_d = (int32_t)(d.stamps[2u * donor + 1u] - t0), gen_d = (int32_t)(d.stamps[2u * donor] - t0);
    const int32_t end_r = (int32_t)(d.stamps[2u * receiver + 1u] - t0);
    const bool pays = end_d - end_r > end_d - gen_d && end_d - gen_d >= 0;
    const bool ok = pays && d.len[donor] > 1u && d.len[receiver] + 2u <= d.row_cap;
    if (ok) deal_move_last(d, donor, receiver);
    d.log[2u * slot] = ok ? donor : kDealEnd;
    d.log[2u * slot + 1u] = receiver;
    return ok;
}

// One learning step after a replayed frame (no-op once learning is over), in two parts: deal_step for every list -- a workgroup
// each, they read the state words and none writes them -- then deal_commit, which does.  bal: the schedule's balance words -- the frame's start
// stamp, the sampled workgroup stamps and the claiming kernel's best time for this view, all in the same ticks.
// scratch: 2 * kDealMaxListWaves + nt words of the workgroup's.
// Keep-best as balance_step does: every stepped frame's time is noted (the seed's own frame counts) and the frame that beats the
// best so far remembered; the last step puts that frame's table back -- it undoes the later steps' moves from the log, last
// step first -- and gives the verdict: a view never rests on a deal that was slower than the claims it replaces.
template <typename Sync>
SVO_DEAL_HD inline void deal_step(const Deal &d, const uint32_t *bal, uint32_t *scratch, uint32_t l, uint32_t tid, uint32_t nt, Sync sync) {
    const uint32_t n = d.state[kDealStep];
    if (n >= kDealLearnFrames || d.state[kDealVerdict] != 0u) return;
    const uint32_t best_before = d.state[kDealBestTime], t0 = bal[kDealBalStart];
    const uint32_t n_rows = d.grid_blocks * 4u;
    uint32_t *const t_of = scratch, *const by_rank = scratch + kDealMaxListWaves, *const red = scratch + 2u * kDealMaxListWaves;
    // the frame's time: the latest wave, and the latest of the sampled workgroup stamps
    uint32_t mine = 0u;
    for (uint32_t w = tid; w < n_rows; w += nt) {
        const uint32_t t = d.stamps[2u * w + 1u] - t0;
        if (deal_valid_time(t) && t > mine) mine = t;
    }
    const uint32_t t_frame = deal_reduce_max(red, mine, tid, nt, sync);
    const uint32_t t_sample = deal_sample_time(bal, red, tid, nt, sync);
    const bool is_best = t_frame != 0u && (n == 0u || best_before == 0u || t_frame < best_before);
    const bool last = n + 1u == kDealLearnFrames;
    const uint32_t best_step = is_best ? n : d.state[kDealBestStep];
    auto pairs_of = [&](uint32_t w) -> uint32_t {
        uint32_t pairs = w / (d.pairs_div ? d.pairs_div : kDealPairsDiv);
        pairs = pairs < 1u ? 1u : pairs;
        return pairs > w / 2u ? w / 2u : pairs;
    };
    uint32_t moved = 0u;
    if (last) {
        for (uint32_t s = n; s-- > best_step;) {  // frame best_step was traced before the moves of steps best_step .. n - 1
            for (uint32_t p = tid; p < pairs_of(deal_list_waves(d.grid_blocks, l)); p += nt) {
                const uint32_t slot = deal_log_slot(d.grid_blocks, s, l, p);
                if (d.log[2u * slot] != kDealEnd) deal_move_last(d, d.log[2u * slot + 1u], d.log[2u * slot]);
            }
            sync();
        }
    } else {
        {  // moves never cross lists: a list is one XCD's, and so is its L2
            const uint32_t w = deal_list_waves(d.grid_blocks, l);
            for (uint32_t i = tid; i < w; i += nt) t_of[i] = d.stamps[2u * deal_wave(l, i) + 1u] - t0;
            sync();
            for (uint32_t i = tid; i < w; i += nt) {  // rank by end time, ties by wave
                uint32_t r = 0u;
                for (uint32_t j = 0; j < w; j++) r += (t_of[j] < t_of[i] || (t_of[j] == t_of[i] && j < i)) ? 1u : 0u;
                by_rank[r] = i;
            }
            sync();
            for (uint32_t p = tid; p < pairs_of(w); p += nt) {  // the p-th latest wave gives to the p-th earliest (all different waves)
                // (a frame without a time moves nothing, but its step leaves its log slots empty all the same)
                if (t_frame == 0u) d.log[2u * deal_log_slot(d.grid_blocks, n, l, p)] = kDealEnd;
                else moved += deal_try_move(d, deal_wave(l, by_rank[w - 1u - p]), deal_wave(l, by_rank[p]), t0, deal_log_slot(d.grid_blocks, n, l, p)) ? 1u : 0u;
            }
            sync();
        }
    }
    red[tid] = moved;
    sync();
    if (tid == 0u) {
        uint32_t m = 0u;
        for (uint32_t i = 0; i < nt; i++) m += red[i];
        d.state[kDealTmpMoves + l] = m;
        if (l == 0u) {
            d.state[kDealTmpTime] = t_frame;
            d.state[kDealTmpSample] = t_sample;
        }
    }
    sync();
}

// ... and what the step found goes into the state words (one thread, after every list's deal_step)
SVO_DEAL_HD inline void deal_commit(const Deal &d, const uint32_t *bal) {
    const uint32_t n = d.state[kDealStep];
    if (n >= kDealLearnFrames || d.state[kDealVerdict] != 0u) return;
    const uint32_t best_before = d.state[kDealBestTime], t_frame = d.state[kDealTmpTime];
    const bool is_best = t_frame != 0u && (n == 0u || best_before == 0u || t_frame < best_before);
    uint32_t m = 0u;
    for (uint32_t l = 0; l < 8u; l++) m += d.state[kDealTmpMoves + l];
    d.state[kDealMoves] += m;
    d.state[kDealLastMoves] = m;
    d.state[kDealLastTime] = t_frame;
    if (is_best) {
        d.state[kDealBestTime] = t_frame;
        d.state[kDealBestSample] = d.state[kDealTmpSample];
        d.state[kDealBestStep] = n;
    }
    d.state[kDealStep] = n + 1u;
    if (n + 1u == kDealLearnFrames) {
        // what replay has to beat: the claiming kernel's best frame of the list-share learning and its last frame from these
        // lists (the first may be another view's when the camera has moved since: the smaller of the two is the safe bar)
        const uint32_t learnt = bal[kDealBalBestTime], recent = d.state[kDealClaimTime], ours = d.state[kDealBestSample];
        const uint32_t claims = learnt != 0u && (recent == 0u || learnt < recent) ? learnt : recent;
        d.state[kDealVerdict] = (ours != 0u && (claims == 0u || ours < claims)) ? 1u : 2u;
    }
}

// ---- the host's part: what a frame launches ----

// What the caller measures for a STACK frame before it is traced.
struct DealFacts {
    bool enabled = false;       // SVO_OPT_STATIC_DEAL
    bool plain_static = false;  // slot 0, a pixel frame, unfiltered, not counting, no fused shadows, no debug buffer, default stack depth
    bool stored_lists = false;  // plan_before_trace traces from the complete stored lists, with the balance words fed
    bool at_rest = false;       // camera and tree are the ones the lists were built from
    uint32_t balance_frames = 0;  // SchedState's, before this frame's post pass
    uint32_t grid_blocks = 0, row_cap = 0;  // of this frame's launch (deal_row_cap; 0: no replay)
    uint32_t seen_step = 0, seen_verdict = 0;  // the device state as the mirror last showed it
    bool seen_fresh = false;    // ... and whether that was read since the last time it was asked for
};

// What the host remembers between frames (the buffers live in svo_ctx::Sched).
struct DealState {
    bool seeded = false;       // the device table belongs to the stored lists and this grid
    bool claims = false;       // the device said "claims": the view is traced by the claiming kernel until its lists are dropped
    uint32_t learn_left = 0;   // replayed frames that still get a step kernel
    uint32_t grid_blocks = 0, row_cap = 0;  // what the table was seeded for
    bool want_mirror = false;  // a copy of the device state is on its way (or wanted)
    uint64_t replayed = 0, seeds = 0;  // frames traced by the replay kernel, seed launches (diagnostics)
};

struct DealPlan {
    bool seed = false;    // seed the table from the stored lists before the trace
    bool replay = false;  // trace with the replay kernel
    bool step = false;    // step kernel after the trace
    bool mirror = false;  // then copy the device state for the host to look at later
};

inline DealPlan deal_before_trace(DealState &s, const DealFacts &f) {
    DealPlan p;
    const bool settled = f.at_rest && f.balance_frames >= kBalanceLearnFrames;
    if (!(f.enabled && f.plain_static && f.stored_lists && settled && f.row_cap != 0u)) {
        const uint64_t replayed = s.replayed, seeds = s.seeds;
        s = DealState{};  // the table is dropped
        s.replayed = replayed;
        s.seeds = seeds;
        return p;
    }
    if (f.seen_fresh && s.want_mirror) {
        s.want_mirror = false;
        if (f.seen_verdict == 2u) s.claims = true;
        if (f.seen_step >= kDealLearnFrames) s.learn_left = 0;  // (a compare that kept the table: nothing to learn again)
    }
    if (!s.seeded || s.grid_blocks != f.grid_blocks || s.row_cap != f.row_cap) {
        s.seeded = true;
        s.claims = false;
        s.learn_left = kDealLearnFrames;
        s.grid_blocks = f.grid_blocks;
        s.row_cap = f.row_cap;
        s.want_mirror = false;
        s.seeds++;
        p.seed = true;
    }
    if (s.claims) return p;
    p.replay = true;
    s.replayed++;
    if (s.learn_left != 0u) {
        p.step = true;
        s.learn_left--;
        if (s.learn_left == 0u) p.mirror = s.want_mirror = true;  // the verdict
    }
    return p;
}

// After the post pass of a frame whose view has a table: lists rebuilt from the same input are compared with the table's own
// on the device (the host launches that unconditionally); the step kernels of the next frames are no-ops unless it re-seeded.
inline bool deal_after_post(DealState &s, const DealPlan &p, bool lists_rebuilt, bool &mirror) {
    mirror = p.mirror;
    if (!(s.seeded && lists_rebuilt)) return false;
    if (!s.claims) {
        s.learn_left = kDealLearnFrames;
        mirror = s.want_mirror = true;
    }
    return !s.claims;
}

}  // namespace svo
