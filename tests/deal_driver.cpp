// Drives the static deal's rules (octree-tracer_amd/csrc/svo_deal.h) as one thread, the way svo_deal.hip's kernels drive them as a
// workgroup: seed, step and compare on host arrays, with a model frame in place of the replay kernel (a wave's time is its start
// delay plus the costs of its row's strips; its stamps are taken where the kernel takes them).  Commands on stdin, one per line
// (see tests/test_deal_host.py):
//   grid BLOCKS ORDER_CAP PAIRS_DIV   buffers for that grid; prints "row_cap N" (0: such a frame stays with claims)
//   list L N e0 .. eN-1               list L of the schedule
//   cost STRIP TICKS | delay WAVE TICKS | default_cost TICKS
//   claims_time T | learnt_time T     what the claiming kernel's last frame took / its best of the list-share learning (0: none)
//   seed | frame | stamp WAVE GEN END | step | compare | policy ... | dump
// dump prints "state step best best_sample verdict seeds moves last_time last_moves claim_time", then "row W: entries".
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "svo_deal.h"

int main() {
    std::vector<uint32_t> order, table, len, log, lists, stamps, state(svo::kDealStateWords, 0u), bal(svo::kDealBalHead + svo::kDealBalSlots, 0u);
    std::vector<uint32_t> scratch(2 * svo::kDealMaxListWaves + 1, 0u);
    std::map<uint32_t, uint32_t> cost, delay;
    uint32_t default_cost = 100, claims_time = 0;
    svo::Deal d{};
    svo::DealState host;
    const uint32_t t0 = 1000;
    auto sync = [] {};
    char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        char cmd[64] = {};
        int at = 0;
        if (sscanf(line, "%63s%n", cmd, &at) != 1) continue;
        const char *rest = line + at;
        const std::string c = cmd;
        if (c == "grid") {
            unsigned blocks, cap, div;
            sscanf(rest, "%u %u %u", &blocks, &cap, &div);
            d.grid_blocks = blocks, d.order_cap = cap, d.pairs_div = div;
            d.row_cap = svo::deal_row_cap(cap, blocks);
            order.assign(8 + 8 * cap, 0u);
            lists.assign(8 + 8 * cap, 0u);
            table.assign((size_t)blocks * 4 * (d.row_cap ? d.row_cap : 1), 0xDEADBEEFu);  // (garbage: a seed must not rely on cleared rows)
            len.assign((size_t)blocks * 4, 0xDEADBEEFu);
            log.assign(svo::deal_log_words(blocks), 0xDEADBEEFu);
            stamps.assign((size_t)blocks * 8, 0u);
            d.table = table.data(), d.len = len.data(), d.log = log.data(), d.lists = lists.data(), d.stamps = stamps.data(), d.state = state.data();
            printf("row_cap %u\n", d.row_cap);
        } else if (c == "list") {
            unsigned l, n;
            int used = 0;
            sscanf(rest, "%u %u%n", &l, &n, &used);
            rest += used;
            order[l] = n;
            for (unsigned k = 0; k < n; k++) {
                unsigned e;
                sscanf(rest, "%u%n", &e, &used);
                rest += used;
                order[8 + l * d.order_cap + k] = e;
            }
        } else if (c == "cost" || c == "delay") {
            unsigned k, t;
            sscanf(rest, "%u %u", &k, &t);
            (c == "cost" ? cost : delay)[k] = t;
        } else if (c == "default_cost") {
            sscanf(rest, "%u", &default_cost);
        } else if (c == "claims_time") {
            sscanf(rest, "%u", &claims_time);
        } else if (c == "learnt_time") {
            sscanf(rest, "%u", &bal[svo::kDealBalBestTime]);
        } else if (c == "seed") {
            // the balance words as the claiming kernel's last frame left them: every sampled workgroup ended at claims_time
            bal[svo::kDealBalStart] = t0;
            bal[svo::kDealBalStamps] = d.grid_blocks;
            for (uint32_t b = 0; b < d.grid_blocks; b++) bal[svo::kDealBalHead + b] = t0 + claims_time;
            svo::deal_seed(d, order.data(), claims_time ? bal.data() : nullptr, scratch.data() + 2 * svo::kDealMaxListWaves, 0u, 1u, sync);
        } else if (c == "frame") {  // the replay kernel's stamps for the current table
            bal[svo::kDealBalStart] = t0;
            bal[svo::kDealBalStamps] = d.grid_blocks;
            for (uint32_t w = 0; w < d.grid_blocks * 4; w++) {
                uint32_t t = t0 + (delay.count(w) ? delay[w] : 0u) + 1u, gen = 0u;
                for (uint32_t j = 0; j < d.row_cap && table[w * d.row_cap + j] != svo::kDealEnd; j++) {
                    const uint32_t s = table[w * d.row_cap + j];
                    gen = t;
                    t += cost.count(s) ? cost[s] : default_cost;
                }
                if (gen) stamps[2 * w] = gen;
                stamps[2 * w + 1] = t;
                if (w % 4 == 0) bal[svo::kDealBalHead + w / 4] = t;  // (the workgroup's stamp is its first wave's)
            }
        } else if (c == "stamp") {
            unsigned w, g, e;
            sscanf(rest, "%u %u %u", &w, &g, &e);
            stamps[2 * w] = t0 + g, stamps[2 * w + 1] = t0 + e;
            if (w % 4 == 0) bal[svo::kDealBalHead + w / 4] = t0 + e;
        } else if (c == "step") {
            for (uint32_t l = 0; l < 8; l++) svo::deal_step(d, bal.data(), scratch.data(), l, 0u, 1u, sync);
            svo::deal_commit(d, bal.data());
        } else if (c == "compare") {
            uint32_t flag = 0;
            svo::deal_reseed_if_changed(d, order.data(), &flag, 0u, 1u, sync);
        } else if (c == "policy") {  // enabled plain stored at_rest balance_frames grid row_cap fresh seen_step seen_verdict rebuilt
            svo::DealFacts f;
            unsigned v[11] = {};
            sscanf(rest, "%u %u %u %u %u %u %u %u %u %u %u", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9], &v[10]);
            f.enabled = v[0], f.plain_static = v[1], f.stored_lists = v[2], f.at_rest = v[3], f.balance_frames = v[4];
            f.grid_blocks = v[5], f.row_cap = v[6], f.seen_fresh = v[7], f.seen_step = v[8], f.seen_verdict = v[9];
            const svo::DealPlan p = svo::deal_before_trace(host, f);
            bool mirror = false;
            const bool compare = svo::deal_after_post(host, p, v[10] != 0, mirror);
            printf("plan seed %d replay %d step %d mirror %d compare %d | seeded %d claims %d learn_left %u\n", p.seed, p.replay, p.step, mirror,
                   compare, host.seeded, host.claims, host.learn_left);
        } else if (c == "dump") {
            printf("state %u %u %u %u %u %u %u %u %u\n", state[svo::kDealStep], state[svo::kDealBestTime], state[svo::kDealBestSample],
                   state[svo::kDealVerdict], state[svo::kDealSeeds], state[svo::kDealMoves], state[svo::kDealLastTime], state[svo::kDealLastMoves],
                   state[svo::kDealClaimTime]);
            for (uint32_t w = 0; w < d.grid_blocks * 4; w++) {
                printf("row %u:", w);
                uint32_t j = 0;
                for (; j < d.row_cap && table[w * d.row_cap + j] != svo::kDealEnd; j++) printf(" %u", table[w * d.row_cap + j]);
                printf(j < d.row_cap ? "\n" : " UNTERMINATED\n");
            }
            printf("end\n");
        }
    }
}
