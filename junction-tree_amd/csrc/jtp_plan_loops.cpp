// Planner, unit 3 of 6 (jtp_plan_build.h has the map): the loops of one task - the cost model and its search, the F / A / R split of the
// index bits with every index table of the task (plan_loops), workgroup records and lean records.
#include "jtp_plan_build.h"

namespace {

// ---- layout policy 4: a cost model of one task, searched over loop sets (and, in layouts(), over thread parts) -----
// Made for cliques whose messages are not small beside the table (config 3: 2 MiB messages, 8-64 MiB tables), where
// the greedy F/A/R split below ends at 8 iterations per workgroup under 50-70 KiB of sub-boxes and 8-16 partial
// copies.  The model prices a task as workgroups x (start-up + staging + iterations + epilogues + flush) over the
// workgroups the chip holds, floored by its bytes at streaming speed, plus the reduce tasks of its partial copies.
// The constants are from in-kernel time stamps on config 3 and 4 (profiles/r02_stage_times*.txt): they only have to
// rank candidates, not to predict microseconds.
// Loop order of the A bits (loop bits some outgoing message contains): bits of the fewest outgoing messages first, and
// among those the largest class first, so that the messages which do NOT contain the leading bits keep their sums in
// registers over the longest runs (JtTask::out_run).
void order_a_bits(std::vector<int> &Ab, const std::vector<uint32_t> &outs) {
    auto klass = [&](int b) {
        uint32_t k = 0;
        for (size_t j = 0; j < outs.size(); ++j) k |= (outs[j] >> b & 1u) << j;
        return k;
    };
    int size[1 << JT_MAX_OUT] = {0};
    for (int b : Ab) ++size[klass(b)];
    std::stable_sort(Ab.begin(), Ab.end(), [&](int a, int b) {
        const uint32_t ka = klass(a), kb = klass(b);
        if (popc(ka) != popc(kb)) return popc(ka) < popc(kb);
        if (size[ka] != size[kb]) return size[ka] > size[kb];
        if (ka != kb) return ka < kb;
        return a < b;
    });
}

struct CostK {               // constants of the model (JTP_COST_* environment overrides are experiments only)
    // (round 3, tools/c3_sweep.sh again after the kernel changes of the round: stage_fix 5 -> 8 and red_bw 3e6 -> 5e6 take
    //  config 3 from 12.2 to 11.7 ms - fewer, longer collect workgroups - with configs 2, 4, 5 and the rank share within noise;
    //  7 and 9-10 lose it again: the constants choose among a handful of discrete layouts)
    double wg = 1.5, stage_fix = 8.0, stage_bw = 4096.0, iter_c = 0.45, iter_d = 0.55, epi = 0.5, wave = 1.5, lane = 0.1,
           flush_fix = 1.0, flush_bw = 16384.0, bw = 5.0e6, red_fix = 4.0, red_bw = 5.0e6, overlap = 0.5, max_cu = 4, lds_cap = 150.0 * 1024;
    CostK() {
        auto g = [](const char *n, double &v) { if (const char *e = getenv(n)) v = atof(e); };
        g("JTP_COST_WG", wg), g("JTP_COST_STAGE_FIX", stage_fix), g("JTP_COST_STAGE_BW", stage_bw), g("JTP_COST_ITER_C", iter_c);
        g("JTP_COST_ITER_D", iter_d), g("JTP_COST_EPI", epi), g("JTP_COST_WAVE", wave), g("JTP_COST_LANE", lane);
        g("JTP_COST_FLUSH_FIX", flush_fix), g("JTP_COST_FLUSH_BW", flush_bw), g("JTP_COST_BW", bw), g("JTP_COST_RED_FIX", red_fix);
        g("JTP_COST_RED_BW", red_bw), g("JTP_COST_OVERLAP", overlap), g("JTP_COST_MAX_CU", max_cu), g("JTP_COST_LDS_CAP", lds_cap);
    }
};
const CostK &cost_k() {
    static const CostK k;
    return k;
}

double task_cost_us(const CostEnv &e, const std::vector<uint32_t> &ins, const std::vector<uint32_t> &outs, uint32_t L, long *lds_out = nullptr) {
    const CostK &K = cost_k();
    const uint32_t tmask = (1u << e.TB) - 1u;
    const uint32_t himask = (e.nbits >= 32 ? ~0u : ((1u << e.nbits) - 1u)) & ~tmask;
    const uint32_t F = himask & ~L, cover = tmask | L;
    const int nL = popc(L);
    if (nL < e.min_loop_log2 || nL > e.max_iter_log2 || popc(F) > JT_MAX_HI) return 1e30;
    const double nwg = std::max(1.0, std::ldexp(e.fill, popc(F))), iters = std::ldexp(1.0, nL);
    long lds = e.unit ? 0 : JT_RING_BYTES;
    double stage = 0, flush = 0, red_bytes = 0, epi = 0;
    int n_red = 0;
    for (uint32_t m : ins) {
        const int fb = popc(m & cover);
        if (fb > JT_MAX_FREE) return 1e30;
        lds += (8L << fb) + JT_STAGE_SCRATCH;
        stage += 8.0 * (double)(1L << fb);
    }
    uint32_t allout = 0;
    for (uint32_t o : outs) allout |= o;
    std::vector<int> Ab;
    for (int b = e.TB; b < e.nbits; ++b)
        if ((L & allout) >> b & 1) Ab.push_back(b);
    if (outs.size() > 1) order_a_bits(Ab, outs);
    const int nR = popc(L & ~allout);
    const uint32_t wave_bits = 3u << (e.TB - 2), lane_bits = 63u << e.EB;
    for (uint32_t o : outs) {
        const int fb = popc(o & cover);
        if (fb > JT_MAX_FREE) return 1e30;
        lds += 8L << fb;
        flush += 8.0 * (double)(1L << fb);
        const int np = popc(F & ~o);
        if (np > 6) return 1e30;
        if (np >= e.red_log2) {               // many partial copies: a reduce task sums them once
            red_bytes += (std::ldexp(1.0, np) + 1.0) * 8.0 * std::ldexp(1.0, popc(o));
            ++n_red;
        } else if (np) {                      // fewer: the consumers sum the copies while they stage
            red_bytes += std::ldexp(1.0, np) * 8.0 * std::ldexp(1.0, popc(o));
            if (e.chain) ++n_red;             // (on a chain that wait is on the critical path: priced like the reduce hop)
        }
        // an epilogue folds the register sums into the sub-box: butterflies over summed lane bits, one ordered
        // phase (barriers) per summed wave bit; it follows every run of iterations whose loop bits the message lacks
        int run = nR;
        for (int b : Ab) {
            if (o >> b & 1) break;
            ++run;
        }
        epi += std::ldexp(K.epi * (1.0 + K.wave * popc(~o & wave_bits)) + K.lane * popc(~o & lane_bits), nL - run);
    }
    if (lds > e.lds_cap || lds > (long)K.lds_cap) return 1e30;
    if (lds_out) *lds_out = lds;
    const double epilogues = 1.0;          // (epi already holds every message's epilogues of the whole loop)
    // (start-up, staging and flush are latency chains: record -> addresses -> message loads -> LDS -> barrier cost
    //  6-7 us even for a few KiB)
    const double t_wg = K.wg + (ins.empty() ? 0.0 : K.stage_fix) + stage / K.stage_bw + iters * (e.dist ? K.iter_d : K.iter_c) + epilogues * epi +
                        (outs.empty() ? 0.0 : K.flush_fix) + flush / K.flush_bw;
    // (workgroups a CU holds: LDS, and the kernels' registers - four waves per SIMD)
    const int per_cu = (int)std::min((long)K.max_cu, std::max(1L, 160L * 1024 / (lds + 128)));
    const double conc = std::max(1.0, 256.0 * per_cu * e.share);
    const double t_lat = std::max(t_wg, nwg * t_wg / conc);
    const double bytes = nwg * (e.unit ? 0.0 : iters * 4096.0 * (e.dist ? 2.0 : 1.0)) + nwg * (0.5 * stage + flush);
    // (neither bound hides the other completely: a workgroup's start-up and epilogues issue no loads)
    const double t_bw = bytes / (K.bw * e.share);
    double t = std::max(t_lat, t_bw) + K.overlap * std::min(t_lat, t_bw);
    if (n_red) t += K.red_fix;
    t += red_bytes / (K.red_bw * e.share);
    return t;
}

}  // namespace

void jtp_keep_cost(double &fix_us, double &iter_us, double &bytes_per_us) {
    const CostK &K = cost_k();
    fix_us = K.wg + K.stage_fix + K.flush_fix;
    iter_us = K.iter_d;
    bytes_per_us = K.bw;
}

LoopChoice search_loops(const CostEnv &e, const std::vector<uint32_t> &ins, const std::vector<uint32_t> &outs, bool exhaustive) {
    LoopChoice best;
    const int n = (int)e.units.size();
    auto consider = [&](uint32_t L) {
        long lds = 0;
        const double us = task_cost_us(e, ins, outs, L, &lds);
        if (us < best.us) best.L = L, best.us = us, best.lds = lds;
        return us;
    };
    if (exhaustive) {
        // depth first over the units, low bits first, pruned by the iteration cap
        std::vector<std::pair<int, uint32_t>> stack;      // (next unit, L)
        stack.push_back({0, 0u});
        while (!stack.empty()) {
            auto [i, L] = stack.back();
            stack.pop_back();
            if (i == n) {
                consider(L);
                continue;
            }
            stack.push_back({i + 1, L});
            if (popc(L | e.units[i]) <= e.max_iter_log2) stack.push_back({i + 1, L | e.units[i]});
        }
    } else {
        uint32_t L = 0;
        for (;;) {
            int pick = -1;
            double pick_us = 1e31;
            for (int i = 0; i < n; ++i) {
                if ((L & e.units[i]) || popc(L | e.units[i]) > e.max_iter_log2) continue;
                const double us = popc(L | e.units[i]) < e.min_loop_log2 ? 1e30 : consider(L | e.units[i]);
                // (below four iterations nothing can be priced: take the unit the fewest messages contain)
                double key = us;
                if (us >= 1e30) {
                    int cnt = 0;
                    for (uint32_t m : ins) cnt += (m & e.units[i]) != 0;
                    for (uint32_t o : outs) cnt += 2 * ((o & e.units[i]) != 0);
                    key = 1e30 + cnt;
                }
                if (key < pick_us) pick_us = key, pick = i;
            }
            if (pick < 0) break;
            L |= e.units[pick];
        }
    }
    return best;
}

namespace {

// Does the high part (bits >= TB) of logical index `x`, restricted to the bits in `within`, name rows that exist?
// A compact variable whose bits all lie in `within` must have a digit below its cardinality; a padding bit in
// `within` must be clear.  (Variables only partly in `within` cannot occur: their bits stay together.)
bool high_digits_exist(const PNode &p, uint32_t x, uint32_t within) {
    if (x & within & p.pad_mask) return false;
    for (size_t g = 0; g < p.group_mask.size(); ++g) {
        if ((p.group_mask[g] & within) != p.group_mask[g]) continue;
        if ((int)((x & p.group_mask[g]) >> p.group_pos[g]) >= p.group_card[g]) return false;
    }
    return true;
}

}  // namespace

int plan_loops(const HostPlan &hp, const PNode &p, JtTask &tk, std::vector<int32_t> &itab, const std::vector<MsgView> &ins,
               const std::vector<MsgView> &outs, int block_log2, std::string &err, int strict_budget, double share) {
    const int TB = hp.TB, nbits = p.nbits;
    int real_bits = 0;                           // (index bits that belong to variables: the others are padding)
    for (int nb : p.nb) real_bits += nb;
    // the bits of a compact variable (stored at its true cardinality) go to the chunk bits or stay loop bits TOGETHER
    auto unit = [&](int b) {
        for (uint32_t g : p.group_mask)
            if (g >> b & 1) return g;
        return 1u << b;
    };
    // strict_budget (multi-set plans): the sub-boxes of ONE evidence set must fit in that many bytes, whatever
    // it costs in loop iterations (down to 4) - the kernel reserves exactly that much LDS per set
    const int budget = strict_budget > 0 ? strict_budget : (hp.lds_budget > 0 ? hp.lds_budget : 32 * 1024);
    // at most 8 partial copies per outgoing message; small levels (few cliques) may use up to 64
    // so that a lone clique still spreads over >= 128 workgroups
    const int PMAX_LOG2 = block_log2 <= 13 ? 6 : 3;
    const uint32_t himask = nbits >= 32 ? 0 : (((1u << nbits) - 1) & ~((1u << TB) - 1));
    uint32_t allout = 0, everyout = himask;
    for (auto &o : outs) {
        allout |= o.mask;
        everyout &= o.mask;
    }
    if (outs.empty()) everyout = 0;

    auto lds_of = [&](uint32_t F) {
        long total = 0;
        for (auto &m : ins) total += 8L << popc(m.mask & ~F);
        for (auto &m : outs) total += 8L << popc(m.mask & ~F);
        return total;
    };
    auto max_free = [&](uint32_t F) {
        int mx = 0;
        for (auto &m : ins) mx = std::max(mx, popc(m.mask & ~F));
        for (auto &m : outs) mx = std::max(mx, popc(m.mask & ~F));
        return mx;
    };
    auto part_log2 = [&](uint32_t F) {       // worst partial count over the outputs
        int mx = 0;
        for (auto &o : outs) mx = std::max(mx, popc(F & ~o.mask));
        return mx;
    };

    uint32_t F = 0;
    bool searched = false;
    if (p.layout == 4 && strict_budget == 0) {
        // searched split (cost model above): every loop set the iteration cap allows
        CostEnv e;
        e.TB = TB, e.EB = hp.EB, e.nbits = nbits, e.dist = tk.mode == 1, e.share = share, e.unit = tk.unit != 0;
        e.red_log2 = hp.knobs.reduce_min >= 0 ? std::max(0, ceil_log2(std::max(hp.knobs.reduce_min, 1))) : (hp.chain_plan ? 3 : 6);
        e.chain = hp.chain_plan;
        e.min_loop_log2 = hp.chain_plan ? JT_MIN_LOOP_LOG2 : JT_MIN_ITER_LOG2;
        e.max_iter_log2 = std::min(std::max(block_log2 - TB, JT_MIN_ITER_LOG2), JT_MAX_ITER_LOG2);
        if (hp.knobs.top_min_loop > 0 && share >= hp.knobs.top_share && !hp.chain_plan) {
            // levels of at most eight cliques (a clique holding >= 12 % of its level): workgroups of at least 8 rows, not 4,
            // so that the workgroups of two or three such levels are resident at once with their rows in flight - as on a
            // chain - instead of one level filling every slot of the chip and the next paying its start-up behind it.
            // A/B on one box, three times: rank share of config 4 at 8 ranks 196 -> 192.5 us, config 4 on one GPU +-0
            // (16 rows: 0.601 -> 0.631 ms, 216 us; 32 rows: 0.665 ms)
            e.min_loop_log2 = std::max(e.min_loop_log2, std::min(hp.knobs.top_min_loop, nbits - TB));
            e.max_iter_log2 = std::max(e.max_iter_log2, e.min_loop_log2);
            // ... and levels of at most 2048 rows in all (one or two cliques of config 4): exactly FOUR rows, the depth of the
            // element ring - every row of such a workgroup is in flight while it waits for its messages, where rows 5-8 of
            // an eight-row workgroup are only asked for once the loop runs (2.2-3.0 us of every hand-over at the top of a tree,
            // profiles/r03_stage_times_rank0_of_8.txt "more steps"), and one or two such levels still leave room for the next
            // (at most 512 workgroups).  A/B on one box: a rank's share of config 4 at 8 ranks 198.7 -> 189.3 us, config 4
            // 0.5981 -> 0.5948 ms; two rows: 210 us.  Larger levels of few cliques (config 3: 64 MiB tables) keep their long workgroups:
            // held to four rows they took 19.7 instead of 11.7 ms.
            const double lvl_rows = (double)p.phys_elems / std::max(share, 1e-9) / (double)(1 << TB);
            if (hp.knobs.top_rows2 > 0 && lvl_rows <= hp.knobs.top_rows2 && nbits - TB >= hp.knobs.top_loop2) {
                e.min_loop_log2 = std::max(hp.knobs.top_loop2, JT_MIN_LOOP_LOG2);
                e.max_iter_log2 = std::max(hp.knobs.top_loop2, JT_MIN_LOOP_LOG2);
            }
        }
        if (hp.lds_budget > 0) e.lds_cap = (tk.unit ? 0 : JT_RING_BYTES) + hp.lds_budget + JT_STAGE_SCRATCH * (long)ins.size();
        uint32_t seen = 0;
        for (int b = TB; b < nbits; ++b)
            if (!(seen >> b & 1)) e.units.push_back(unit(b)), seen |= unit(b);
        for (size_t g = 0; g < p.group_mask.size(); ++g) e.fill *= (double)p.group_card[g] / (double)(1 << popc(p.group_mask[g]));
        e.fill = std::ldexp(e.fill, -popc(p.pad_mask & himask));
        std::vector<uint32_t> im, om;
        for (auto &m : ins) im.push_back(m.mask);
        for (auto &o : outs) om.push_back(o.mask);
        LoopChoice ch = search_loops(e, im, om, true);
        if (getenv("JTP_PLAN_DEBUG") && nbits >= 24) {
            fprintf(stderr, "pnode %d mode %d nbits %d cap %d share %.3f best L %x us %.1f lds %ld\n", tk.pnode, tk.mode, nbits, e.max_iter_log2, e.share, ch.L, ch.us, ch.lds);
            for (int k = 2; k <= 6; ++k) { CostEnv e2 = e; e2.max_iter_log2 = k; LoopChoice c2 = search_loops(e2, im, om, true); fprintf(stderr, "   cap %d: L %x us %.1f lds %ld\n", k, c2.L, c2.us, c2.lds); }
        }
        if (ch.us < 1e30) F = himask & ~ch.L, searched = true;
    }
    // 1. LDS must fit: fix the high bit that shrinks the staged sub-boxes most.
    bool down_to_four = strict_budget > 0;
    while (!searched && (lds_of(F) > budget || max_free(F) > JT_MAX_FREE)) {
        int best = -1;
        long best_lds = 0;
        int best_part = 0;
        for (int b = TB; b < nbits; ++b) {      // (fitting LDS never goes below 8 iterations: staging a big
                                                //  sub-box for 4 would cost more than it saves; multi-set plans: 4 - and 4
                                                //  for anybody whose sub-boxes do not fit at all otherwise, see below)
            if (F >> b & 1) continue;
            if (nbits - popc(F | unit(b)) < TB + (down_to_four ? 2 : 3)) continue;
            long l = lds_of(F | unit(b));
            int pl = part_log2(F | unit(b));
            if (best < 0 || l < best_lds || (l == best_lds && pl < best_part)) {
                best = b, best_lds = l, best_part = pl;
            }
        }
        if (best < 0 || best_lds >= lds_of(F)) {
            if (strict_budget > 0) FAIL(JTP_EUNSUPPORTED, "message sub-boxes of one evidence set need %ld bytes of LDS (limit %d)", lds_of(F), strict_budget);
            // cannot shrink further: accepted while the whole workgroup - ring, sub-boxes, staging scratch and the kernels'
            // static words - stays inside the CU's 160 KiB (150 KiB of sub-boxes alone, the bound of rounds 1-2, did not:
            // hipFuncSetAttribute refused 170 KiB on a random factor graph, tools/gpu_fuzz_api.py)
            // (4 KiB for the static words: the reduce path's 2 KiB of partial sums and the dataflow control words are in the same kernels)
            if (lds_of(F) + (tk.unit ? 0 : JT_RING_BYTES) + JT_STAGE_SCRATCH * (long)ins.size() + 4096 <= 160 * 1024 && max_free(F) <= JT_MAX_FREE) break;
            // (a marginal onto nearly all variables of a clique of few rows - a factor as wide as its clique, 3^8 entries:
            //  four rows per workgroup before giving up)
            if (!down_to_four) {
                down_to_four = true;
                continue;
            }
            FAIL(JTP_EUNSUPPORTED, "message sub-boxes do not fit in LDS (%ld bytes)", lds_of(F));
        }
        F |= unit(best);
    }
    // 2. Parallelism: split until a workgroup handles at most 2^block_log2 elements, preferring
    //    bits that every outgoing message contains (no partial copies), highest bit first.
    block_log2 = std::max(block_log2, TB + JT_MIN_ITER_LOG2);   // a workgroup always runs >= 4 iterations
    block_log2 = std::min(block_log2, TB + JT_MAX_ITER_LOG2);   // and at most 2^JT_MAX_ITER_LOG2
    while (!searched && nbits - popc(F) > block_log2) {
        int best = -1;
        auto fits = [&](int b) { return nbits - popc(F | unit(b)) >= TB + JT_MIN_ITER_LOG2; };      // >= 4 iterations stay
        for (int b = nbits - 1; b >= TB; --b)
            if (!(F >> b & 1) && (everyout & unit(b)) == unit(b) && fits(b)) {
                best = b;
                break;
            }
        if (best < 0) {
            // otherwise: a bit of SOME outgoing message first (left in the loops it would be an A
            // bit, i.e. an epilogue per iteration, whereas bits of no outgoing message make the free
            // register-summed R loop), then fewest partial copies, then the bit most incoming
            // messages contain (smaller staged sub-boxes), then the highest
            int best_pl = 1 << 30, best_in = -1, best_cls = 9;
            for (int b = nbits - 1; b >= TB; --b) {
                if ((F >> b & 1) || !fits(b)) continue;
                int pl = part_log2(F | unit(b));
                int cls = (allout >> b & 1) ? 0 : 1;
                int nin = 0;
                for (auto &m : ins) nin += (m.mask >> b) & 1;
                if (cls < best_cls || (cls == best_cls && (pl < best_pl || (pl == best_pl && nin > best_in))))
                    best_cls = cls, best_pl = pl, best_in = nin, best = b;
            }
            if (best < 0) break;
            if (best_pl > PMAX_LOG2 && nbits - popc(F) <= TB + JT_MAX_ITER_LOG2) break;
        }
        F |= unit(best);
    }
    if (popc(F) > JT_MAX_HI) FAIL(JTP_EUNSUPPORTED, "too many chunk bits (%d)", popc(F));
    if (nbits - popc(F) > TB + JT_MAX_ITER_LOG2)
        FAIL(JTP_EUNSUPPORTED, "cannot split a table of %d index bits into workgroups of at most 64 rows without splitting a "
                               "variable stored at its true cardinality", nbits);

    std::vector<int> Fb, Ab, Rb;
    for (int b = TB; b < nbits; ++b) {
        if (F >> b & 1) Fb.push_back(b);
        else if (allout >> b & 1) Ab.push_back(b);
        else Rb.push_back(b);
    }
    {
        std::vector<uint32_t> om;
        for (auto &o : outs) om.push_back(o.mask);
        order_a_bits(Ab, om);
    }
    tk.nbits = nbits;
    tk.tmap_off = (hp.tmix || tk.unit) ? p.tmap_off : -1;      // (unit tasks: which entries of a row exist)
    tk.vgroups = (hp.tmix && !tk.unit && !p.vmap.empty()) ? 2 : 0;
    if (hp.tmix_compact && !tk.unit && tk.vgroups != 2) FAIL(JTP_EUNSUPPORTED, "internal: a task of clique %d without its list of logical threads in a compact plan", p.real);
    tk.real_bits = real_bits;
    tk.debug = hp.knobs.debug;
    tk.nF = (int)Fb.size();
    tk.nA = (int)Ab.size();
    tk.nR = (int)Rb.size();
    tk.n_in = (int)ins.size();
    tk.n_out = (int)outs.size();
    if (tk.nA > JT_MAX_HI || tk.nR > JT_MAX_HI) FAIL(JTP_EUNSUPPORTED, "too many loop bits");
    for (int j = 0; j < tk.nF; ++j) {
        tk.f_x[j] = (uint32_t)p.bitw[Fb[j]];
        tk.f_lx[j] = 1u << Fb[j];
    }
    for (int t = 0; t < tk.nR; ++t) tk.loop_pos[t] = (uint8_t)Rb[t];
    for (int t = 0; t < tk.nA; ++t) tk.loop_pos[tk.nR + t] = (uint8_t)Ab[t];
    tk.out_run = 0;
    for (size_t j = 0; j < outs.size(); ++j) {
        int run = tk.nR;
        for (int b : Ab) {
            if (outs[j].mask >> b & 1) break;
            ++run;
        }
        tk.out_run |= (uint32_t)run << (8 * j);
    }
    uint32_t loopmask = 0;
    for (int b : Rb) loopmask |= 1u << b;
    for (int b : Ab) loopmask |= 1u << b;

    int lds = tk.unit ? 0 : JT_RING_BYTES;      // the element ring sits at LDS offset 0 (unit tasks load no rows: no ring)
    // per-message tables
    std::vector<std::vector<int>> slotw;      // [msg][clique bit] -> sub-box slot weight
    auto fill_msg = [&](JtMsg &jm, const MsgView &mv, bool is_out) {
        std::vector<int> sw(32, 0);
        // free message bits = images of clique bits outside F, ascending message bit
        std::vector<std::pair<int, int>> fr;   // (message bit, clique bit)
        for (int b = 0; b < nbits; ++b)
            if ((mv.mask >> b & 1) && !(F >> b & 1)) fr.push_back({mv.dst[b], b});
        std::sort(fr.begin(), fr.end());
        // Sub-box slot order: the index bits that are LANE bits of the clique's thread part come first, the others follow in
        // message order.  The lanes of a half-wave then read one contiguous run of the sub-box (ds_read_b64: 32 lanes x 8 bytes
        // over 64 banks - conflict-free inside 256 bytes), whatever place those variables have in the message; in message order
        // a lane bit of weight >= 32 entries put two lanes on one bank (SQ_LDS_BANK_CONFLICT: a third of all LDS cycles of
        // jt_multi_flow).  64 evidence sets 6.04 -> 5.32 ms, 8 sets 1.02 -> 0.89, config 3 11.78 -> 11.56, configs 2 and 4
        // unchanged (A/B on one box).  Staging and flush follow free_pos[] as before: their global accesses are less contiguous
        // now, which the loop's gain outweighs (slot orders that kept the lowest message bits low measured slower: 5.58 ms).
        // Mixed-radix thread parts have no lane bits: message order.  JTP_LANE_LOW=0: message order, 1: incoming sub-boxes only.
        if (hp.knobs.lane_low > (is_out ? 1 : 0) && !hp.tmix)
            std::stable_partition(fr.begin(), fr.end(), [&](const std::pair<int, int> &x) { return x.second >= hp.EB && x.second < hp.EB + 5; });
        jm.nfree = (int)fr.size();
        jm.src_task = -1;
        for (size_t r = 0; r < fr.size(); ++r) {
            jm.free_pos[r] = (uint8_t)fr[r].first;
            sw[fr[r].second] = 1 << r;
        }
        for (int e = 0; e < 2; ++e) jm.e_w[e] = (e < hp.EB) ? sw[e] : 0;
        for (int t = 0; t < 8; ++t) jm.t_w[t] = sw[hp.EB + t];
        jm.e_dep = 0;
        for (int e = 0; e < hp.EB; ++e) jm.e_dep |= (mv.mask >> e & 1);
        jm.red_e = jm.red_lane = jm.red_wave = 0;
        if (is_out) {
            for (int e = 0; e < hp.EB; ++e) if (!(mv.mask >> e & 1)) jm.red_e |= 1 << e;
            for (int t = 0; t < 6; ++t) if (!(mv.mask >> (hp.EB + t) & 1)) jm.red_lane |= 1 << t;
            for (int t = 0; t < 2; ++t) if (!(mv.mask >> (hp.EB + 6 + t) & 1)) jm.red_wave |= 1 << t;
        }
        int pbit = 0;
        for (int j = 0; j < tk.nF; ++j) {
            int b = Fb[j];
            jm.f_w[j] = (mv.mask >> b & 1) ? (1 << mv.dst[b]) : 0;
            jm.f_p[j] = 0;
            if (is_out && !(mv.mask >> b & 1)) jm.f_p[j] = 1 << pbit++;
        }
        jm.npart = is_out ? (1 << pbit) : 1;      // incoming npart is patched in later
        jm.pstride = 1 << mv.msg_bits;
        jm.lds_off = lds;
        lds += 8 << jm.nfree;
        lds = (lds + 15) & ~15;
        slotw.push_back(sw);
    };
    for (int k = 0; k < tk.n_in; ++k) fill_msg(tk.msg[k], ins[k], false);
    for (int k = tk.n_in; k < JT_MAX_IN; ++k) slotw.push_back(std::vector<int>(32, 0));
    for (int k = 0; k < tk.n_out; ++k) fill_msg(tk.msg[JT_MAX_IN + k], outs[k], true);
    for (int k = tk.n_out; k < JT_MAX_OUT; ++k) slotw.push_back(std::vector<int>(32, 0));

    // iteration table: row i = (a, r), r the fast counter; column 0 = element offset, 1..4 = slot
    // offsets into the incoming sub-boxes, 5..7 = into the outgoing sub-boxes (A bits only)
    tk.total = 1 << (tk.nA + tk.nR);
    itab.assign((size_t)tk.total * JT_NCOL, 0);
    for (int i = 0; i < tk.total; ++i) {
        const int r = i & ((1 << tk.nR) - 1), a = i >> tk.nR;
        int64_t row[JT_NCOL] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t lx = 0;                                    // logical index of the row's loop bits
        for (int t = 0; t < tk.nR; ++t)
            if (r >> t & 1) {
                row[0] += p.bitw[Rb[t]];
                lx |= 1u << Rb[t];
                for (int c = 1; c < JT_NCOL; ++c) row[c] += slotw[c - 1][Rb[t]];
            }
        for (int t = 0; t < tk.nA; ++t)
            if (a >> t & 1) {
                row[0] += p.bitw[Ab[t]];
                lx |= 1u << Ab[t];
                for (int c = 1; c < JT_NCOL; ++c) row[c] += slotw[c - 1][Ab[t]];
            }
        if (!high_digits_exist(p, lx, loopmask)) row[0] = (int64_t)JT_NO_ROW;      // read the zero row instead
        for (int c = 0; c < JT_NCOL; ++c) itab[(size_t)i * JT_NCOL + c] = (int32_t)(uint32_t)row[c];
        if (i < 8) tk.first_x[i] = (uint32_t)row[0];
    }
    if (hp.tmix) {
        // Plans with mixed-radix rows (kernels *_mix) loop over the rows that EXIST only: with cardinality 5 in three bits a
        // loop of two variables is 25 rows, not 64.  Row r of the table is then the r-th existing row, and what the kernels
        // of the other plans derive from the loop counter travels in the upper half of column 1 + JT_MAX_IN: bits 16-21 the
        // row's counter value in the full loop nest (its logical index bits: evidence), bit 24 + j "outgoing message j's
        // run of rows ends here" (JtTask::out_run counts rows of the full nest).
        std::vector<int> live;
        for (int i = 0; i < tk.total; ++i)
            if ((uint32_t)itab[(size_t)i * JT_NCOL] != JT_NO_ROW) live.push_back(i);
        if (live.empty()) FAIL(JTP_EINVAL, "internal: a loop nest without rows");
        std::vector<int32_t> packed(live.size() * JT_NCOL);
        for (size_t r = 0; r < live.size(); ++r) {
            const int i = live[r];
            for (int c = 0; c < JT_NCOL; ++c) packed[r * JT_NCOL + c] = itab[(size_t)i * JT_NCOL + c];
            uint32_t w = (uint32_t)packed[r * JT_NCOL + 1 + JT_MAX_IN];
            if (w >= (1u << 16)) FAIL(JTP_EINVAL, "internal: sub-box offset %u does not fit 16 bits", w);
            w |= (uint32_t)i << 16;
            for (int j = 0; j < tk.n_out; ++j) {
                const int run = (tk.out_run >> (8 * j)) & 0xff;
                if (r + 1 == live.size() || (live[r + 1] >> run) != (i >> run)) w |= 1u << (24 + j);
            }
            packed[r * JT_NCOL + 1 + JT_MAX_IN] = (int32_t)w;
        }
        itab.swap(packed);
        tk.total = (int)live.size();
        for (int i = 0; i < 8; ++i) tk.first_x[i] = i < tk.total ? (uint32_t)itab[(size_t)i * JT_NCOL] : JT_NO_ROW;
    }
    tk.itab_lds = ((lds + 15) & ~15) + JT_STAGE_SCRATCH * tk.n_in;        // sub-boxes, staging scratch per incoming message
    tk.lds_bytes = tk.itab_lds;                           // (the iteration table is register resident)
    if (strict_budget > 0) {
        // element bits in no message of the task: the elements of a 16-byte vector can be summed before they meet
        // the message product (JtTask::esum bit 0; bit 1 - no evidence on those bits - is the engine's)
        bool e_free = !outs.empty();
        for (int k = 0; k < tk.n_in; ++k) e_free = e_free && !tk.msg[k].e_dep;
        for (int k = 0; k < tk.n_out; ++k) e_free = e_free && tk.msg[JT_MAX_IN + k].red_e == (1 << hp.EB) - 1;
        tk.esum = e_free ? 1 : 0;
        if (lds - JT_RING_BYTES > strict_budget) FAIL(JTP_EUNSUPPORTED, "sub-boxes of one evidence set: %d bytes (limit %d)", lds - JT_RING_BYTES, strict_budget);
        tk.setb = strict_budget;
        tk.lds_bytes = JT_RING_BYTES + JT_MSETS * strict_budget;       // ring + one region per evidence set
    }
    return JTP_OK;
}

// ------------------------------------------------------------------------------------------

JtBlock jtp_make_block(const HostPlan &hp, const JtTask &tk, uint32_t task_index, uint32_t chunk) {
    JtBlock b;
    memset(&b, 0, sizeof b);
    b.task = task_index;
    uint32_t fmask = 0;
    for (int j = 0; j < tk.nF; ++j) {
        fmask |= tk.f_lx[j];
        if (!((chunk >> j) & 1u)) continue;
        b.xF += tk.f_x[j];
        b.lxF += tk.f_lx[j];
        for (int k = 0; k < JT_MAX_MSG; ++k) b.gbase[k] += tk.msg[k].f_w[j];
        for (int k = 0; k < JT_MAX_OUT; ++k) b.pnum[k] += tk.msg[JT_MAX_IN + k].f_p[j];
    }
    b.psi_x0 = tk.psi_off + (int64_t)b.xF;
    for (int i = 0; i < 8; ++i) b.first_x[i] = tk.first_x[i];
    // a chunk whose own digits do not exist (a compact variable's digit beyond its cardinality, a padding bit set)
    // has no rows: the workgroup runs on the zero row and writes its all-zero partial copy (jtp_internal.h)
    if (tk.kind == 0 && tk.keep_rows) b.flags |= JT_BLOCK_KEEP_ROWS;
    if (tk.kind == 0 && !high_digits_exist(hp.pn[tk.pnode], b.lxF, fmask)) {
        b.flags |= JT_BLOCK_INVALID;
        b.xF = 0;
        b.psi_x0 = 0;
        for (int i = 0; i < 8; ++i) b.first_x[i] = JT_NO_ROW;
    }
    return b;
}

// The lean record of a unit task (JtLean, jtp_internal.h), appended to `itab` at a 64-byte boundary; JtTask::lean_off says where
// (0: the task runs the generic pass - it keeps a table, has several outputs, stores a belief, belongs to a plan with mixed-radix
// rows or to a multi-set plan, or stages a message of several partial copies).  JTP_NO_LEAN=1: no task gets one.
void jtp_make_lean(const HostPlan &hp, JtTask &tk, std::vector<int32_t> &itab, bool readout) {
    tk.lean_off = 0;
    if (hp.knobs.no_lean || hp.tmix || (hp.multiset && !readout)) return;
    // (tasks of a propagate: one outgoing message, at most three incoming tables - ten row loops in the dataflow kernels; read-out
    //  tasks, whose kernel is off the hot path: up to three marginals of psi x ALL incoming tables of a unit clique)
    const int max_in = readout ? JT_MAX_IN : 3, max_out = readout ? JT_MAX_OUT : 1;
    if (tk.kind != 0 || !tk.unit || tk.mode != 0 || tk.n_out < 1 || tk.n_out > max_out || tk.n_in > max_in || tk.bel_off >= 0 || tk.vgroups) return;
    // (incoming messages of several partial copies: the generic pass splits the copies of a small sub-box over the threads, which the
    //  lock-step staging of the lean pass does not - measured slower inside a propagate; the read-out kernel takes them, copy after copy)
    if (!readout)
        for (int k = 0; k < tk.n_in; ++k)
            if (tk.msg[k].npart != 1) return;
    if ((tk.debug & ~2) != 0) return;                 // (the JTP_DEBUG timing experiments are switches of the generic pass)
    JtLean ln;
    JtLeanMore more;
    memset(&ln, 0, sizeof ln);
    memset(&more, 0, sizeof more);
    auto fill = [&](JtLeanMsg &lm, const JtMsg &m, int src) {
        lm.off = m.off;
        lm.nfree = m.nfree;
        lm.lds_off = m.lds_off;
        lm.flags = (m.same_launch ? 1 : 0) | (m.fixed ? 2 : 0);
        lm.src = src;
        lm.e_w[0] = m.e_w[0], lm.e_w[1] = m.e_w[1];
        for (int b = 0; b < 8; ++b) lm.w_lo[b] = b < m.nfree ? 1 << m.free_pos[b] : 0;
        for (int b = 0; b < 5; ++b) lm.w_hi[b] = 8 + b < m.nfree ? 1 << m.free_pos[8 + b] : 0;
        lm.w_hi[5] = m.npart, lm.w_hi[6] = m.pstride, lm.w_hi[7] = 0;
        for (int t = 0; t < 8; ++t) lm.t_w[t] = m.t_w[t];
    };
    int n = 0;
    for (int pass = 0; pass < 2; ++pass)                      // the tables that depend on the element bits first
        for (int k = 0; k < tk.n_in; ++k)
            if ((tk.msg[k].e_dep != 0) == (pass == 0)) fill(ln.in[n++], tk.msg[k], k);
    for (int k = 0; k < tk.n_in; ++k) ln.n_e += tk.msg[k].e_dep ? 1 : 0;
    for (int j = 0; j < tk.n_out; ++j) {
        const JtMsg &mo = tk.msg[JT_MAX_IN + j];
        const int rmask = (1 << ((tk.out_run >> (8 * j)) & 0xffu)) - 1;
        if (j == 0) {
            fill(ln.out, mo, JT_MAX_IN);
            ln.rmask = rmask;
            ln.red_e = mo.red_e, ln.red_lane = mo.red_lane, ln.red_wave = mo.red_wave;
            ln.out_pstride = mo.pstride;
        } else {
            fill(more.out[j - 1], mo, JT_MAX_IN + j);
            more.rmask[j - 1] = rmask;
            more.red_e[j - 1] = mo.red_e, more.red_lane[j - 1] = mo.red_lane, more.red_wave[j - 1] = mo.red_wave;
            more.out_pstride[j - 1] = mo.pstride;
        }
    }
    ln.n_in = tk.n_in;
    ln.n_out = tk.n_out;
    ln.total = tk.total;
    ln.settle = tk.settle;
    ln.tmap_off = tk.tmap_off;
    ln.itab_off = tk.itab_off;
    if (tk.tmap_off >= 0) {
        const int n_t = 1 << hp.TB;
        for (int x = 0; x < n_t; ++x)
            if (itab[(size_t)tk.tmap_off + x] < 0) ln.some_invalid = 1;
    }
    for (int i = 0; i < tk.total; ++i)
        if ((uint32_t)itab[(size_t)tk.itab_off + (size_t)i * JT_NCOL] == JT_NO_ROW) ln.some_norow = 1;
    while (itab.empty() || itab.size() % 16) itab.push_back(0);
    tk.lean_off = (int64_t)itab.size();
    const int32_t *w = reinterpret_cast<const int32_t *>(&ln);
    itab.insert(itab.end(), w, w + sizeof ln / 4);
    if (tk.n_out > 1) {
        const int32_t *w2 = reinterpret_cast<const int32_t *>(&more);
        itab.insert(itab.end(), w2, w2 + sizeof more / 4);
    }
}
