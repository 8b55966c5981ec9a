// Planner, unit 2 of 6 (jtp_plan_build.h has the map): the bit order of every clique and separator table.
#include "jtp_plan_build.h"

// Layout policy 4: the variables of the thread part (and their order) chosen by the cost model of plan_loops' search,
// summed over the clique's collect and distribute tasks.  Candidates: every set of variables that fills the thread
// part (cliques of up to 12 variables), else a hill climb from the "traffic first" order by swapping one variable in
// and one out.  Inside the thread part variables of the fewest messages go lowest (element bits that are summed cost
// nothing, wave bits that are summed cost a barrier phase each), as in policy 2.
bool PlanBuilder::searched_order(int c, const std::vector<int> &host, const std::vector<int> &seps, std::vector<int> &order) {
    const PNode &p = hp.pn[c];
    const int n = (int)host.size(), TB = hp.TB;
    if (n == 0 || n > 31) return false;
    std::vector<int> cnt(n, 0), canon(n), rank_of(n);
    const bool has_static = wants_static(p);
    for (int i = 0; i < n; ++i) {
        for (int sp : seps) cnt[i] += find_var(hp.ps[sp].vars, host[i]) >= 0;
        if (has_static) cnt[i] += find_var(p.cover, host[i]) >= 0;
        canon[i] = i;
    }
    auto waste = [&](int i) { return (double)(1 << hp.vbits[host[i]]) / hp.card[host[i]]; };
    std::stable_sort(canon.begin(), canon.end(), [&](int a, int b) { return cnt[a] != cnt[b] ? cnt[a] < cnt[b] : waste(a) < waste(b); });
    for (int r = 0; r < n; ++r) rank_of[canon[r]] = r;
    int total_bits = 0;
    for (int v : host) total_bits += hp.vbits[v];
    if (total_bits <= TB || total_bits > JT_MAX_BITS) return false;           // one workgroup row: nothing to choose; too large: refused by layouts()
    auto bits_of = [&](uint32_t S) {
        int b = 0;
        for (int i = 0; i < n; ++i)
            if (S >> i & 1) b += hp.vbits[host[i]];
        return b;
    };
    auto valid = [&](uint32_t S) {                // fills the thread part, and would not without its last variable
        if (!S) return false;
        int last = -1;
        for (int r = n - 1; r >= 0 && last < 0; --r)
            if (S >> canon[r] & 1) last = canon[r];
        const int b = bits_of(S);
        return b >= TB && b - hp.vbits[host[last]] < TB;
    };
    struct Eval { double us = 1e30; uint32_t Ld = 0, Lc = 0; };
    std::vector<int> idx;                          // scratch: candidate order as indices into host
    auto order_of = [&](uint32_t S) {
        idx.clear();
        for (int r = 0; r < n; ++r) if (S >> canon[r] & 1) idx.push_back(canon[r]);
        for (int r = 0; r < n; ++r) if (!(S >> canon[r] & 1)) idx.push_back(canon[r]);
    };
    std::vector<int> pos(n);
    auto evaluate = [&](uint32_t S) {
        Eval ev;
        order_of(S);
        int bit = 0;
        for (int i : idx) pos[i] = bit, bit += hp.vbits[host[i]];
        CostEnv e;
        e.TB = TB, e.EB = hp.EB, e.nbits = std::max(bit, TB + JT_MIN_ITER_LOG2);
        e.unit = p.unit;
        e.red_log2 = hp.knobs.reduce_min >= 0 ? std::max(0, ceil_log2(std::max(hp.knobs.reduce_min, 1))) : (hp.chain_plan ? 3 : 6);
        e.chain = hp.chain_plan;
        e.min_loop_log2 = hp.chain_plan ? JT_MIN_LOOP_LOG2 : JT_MIN_ITER_LOG2;
        uint32_t grouped = 0;
        for (int i : idx) {
            const int card = hp.card[host[i]], nb = hp.vbits[host[i]];
            if (pos[i] >= TB && (hp.compact || p.unit) && (card & (card - 1)) != 0) {
                const uint32_t g = ((1u << nb) - 1u) << pos[i];
                e.units.push_back(g), grouped |= g;
                e.fill *= (double)card / (double)(1 << nb);
            }
        }
        for (int b = TB; b < e.nbits; ++b)
            if (!(grouped >> b & 1)) e.units.push_back(1u << b);
        if (hp.compact || p.unit) e.fill = std::ldexp(e.fill, -(e.nbits - std::max(bit, TB)));
        std::sort(e.units.begin(), e.units.end());
        if (hp.lds_budget > 0) e.lds_cap = (p.unit ? 0 : JT_RING_BYTES) + hp.lds_budget + JT_STAGE_SCRATCH * 4L;
        uint32_t stat_mask = 0;
        if (has_static)
            for (int v : p.cover) {
                const int i = find_var(host, v);
                if (i >= 0) stat_mask |= ((1u << hp.vbits[v]) - 1u) << pos[i];
            }
        auto mask_of = [&](int sp) {
            uint32_t m = 0;
            for (int v : hp.ps[sp].vars) {
                const int i = find_var(host, v);
                if (i >= 0) m |= ((1u << hp.vbits[v]) - 1u) << pos[i];
            }
            return m;
        };
        std::vector<uint32_t> kids, none;
        for (int k : p.children) kids.push_back(mask_of(hp.pn[k].psep));
        const double elems = std::ldexp(1.0, e.nbits);
        ev.us = 0;
        if (c != hp.root && p.psep >= 0) {
            e.dist = false;
            e.max_iter_log2 = std::min(std::max(block_log2_for(0, p.depth, p.owner, false) - TB, JT_MIN_ITER_LOG2), JT_MAX_ITER_LOG2);
            e.share = std::min(1.0, elems / std::max(elems, lvl_elems[0][p.owner][p.depth]));
            std::vector<uint32_t> cin = kids;
            if (has_static) cin.push_back(stat_mask);
            LoopChoice ch = search_loops(e, cin, {mask_of(p.psep)}, false);
            ev.us += ch.us, ev.Lc = ch.L;
        }
        {
            e.dist = true;
            e.max_iter_log2 = std::min(std::max(block_log2_for(1, p.depth, p.owner, false) - TB, JT_MIN_ITER_LOG2), JT_MAX_ITER_LOG2);
            e.share = std::min(1.0, elems / std::max(elems, lvl_elems[1][p.owner][p.depth]));
            std::vector<uint32_t> ins;
            if (p.psep >= 0) ins.push_back(mask_of(p.psep));
            if (has_static) ins.push_back(stat_mask);
            ins.insert(ins.end(), kids.begin(), kids.end());
            LoopChoice ch = search_loops(e, ins, kids, false);
            ev.us += ch.us, ev.Ld = ch.L;
        }
        return ev;
    };
    uint32_t bestS = 0;
    Eval best;
    if (n <= 12) {
        for (uint32_t S = 1; S < (1u << n); ++S) {
            if (!valid(S)) continue;
            Eval ev = evaluate(S);
            if (ev.us < best.us) best = ev, bestS = S;
        }
    } else {
        uint32_t S = 0;                              // start: the canonical prefix
        for (int r = 0; r < n && bits_of(S) < TB; ++r) S |= 1u << canon[r];
        best = evaluate(S), bestS = S;
        for (int pass = 0; pass < 4; ++pass) {
            bool better = false;
            for (int i = 0; i < n; ++i) {
                if (!(bestS >> i & 1)) continue;
                for (int j = 0; j < n; ++j) {
                    if (bestS >> j & 1) continue;
                    const uint32_t S2 = (bestS & ~(1u << i)) | (1u << j);
                    if (!valid(S2)) continue;
                    Eval ev = evaluate(S2);
                    if (ev.us < best.us) {
                        best = ev, bestS = S2, better = true;
                        break;                       // i has left the set
                    }
                }
            }
            if (!better) break;
        }
    }
    if (best.us >= 1e30) return false;
    // thread part in canonical order; above it the variables the distribute task loops over first (its rows are
    // then consecutive 4 KiB pieces), then the collect task's, then the chunk bits
    order_of(bestS);
    int bit = 0;
    for (int i : idx) pos[i] = bit, bit += hp.vbits[host[i]];
    auto klass = [&](int i) {
        const uint32_t m = ((1u << hp.vbits[host[i]]) - 1u) << pos[i];
        if (pos[i] < TB) return 0;
        return (m & best.Ld) ? 1 : (m & best.Lc) ? 2 : 3;
    };
    std::vector<int> fin = idx;
    std::stable_sort(fin.begin(), fin.end(), [&](int a, int b) { return klass(a) < klass(b); });
    order.clear();
    for (int i : fin) order.push_back(host[i]);
    return true;
}

int PlanBuilder::layouts() {
    // ---- bit layouts ----------------------------------------------------------------------
    // (level sizes from the padded index spaces, for the searched layouts: level_work() recomputes them from the
    //  physical sizes once the layouts are known)
    for (int ph = 0; ph < 2; ++ph) lvl_elems[ph].assign(hp.n_ranks + 1, std::vector<double>(maxdepth + 1, 0.0));
    for (int c = 0; c < NP; ++c) {
        const PNode &p = hp.pn[c];
        int cb = 0;
        for (int v : (p.real >= 0 ? hp.node_vars[p.real] : p.vars)) cb += hp.vbits[v];
        const double e = std::ldexp(1.0, std::max(cb, hp.TB + JT_MIN_ITER_LOG2));
        if (c != hp.root) lvl_elems[0][p.owner][p.depth] += e;
        lvl_elems[1][p.owner][p.depth] += e;
    }
    {
        int tiny = 0;
        for (int c = 0; c < NP; ++c) tiny += lvl_elems[1][hp.pn[c].owner][hp.pn[c].depth] <= hp.knobs.tiny_level_elems;
        hp.chain_plan = 2 * tiny > NP;
    }
    for (int c = 0; c < NP; ++c) {
        PNode &p = hp.pn[c];
        std::vector<int> host = p.real >= 0 ? hp.node_vars[p.real] : p.vars;
        std::vector<int> seps;
        if (p.psep >= 0) seps.push_back(p.psep);
        for (int k : p.children) seps.push_back(hp.pn[k].psep);
        std::vector<int> order;                       // LSB first
        // Policy 0 chooses per clique between the two heuristics below.  "Epilogue first" (policy 3) suits
        // cliques whose messages are small beside the table (C4: 3 x 8 KiB against 4 MiB); "traffic first"
        // (policy 2) those whose messages are not, and chain-like cliques, whose levels are latency bound
        // and gain from fewer partial copies.  Measured crossover on trees of 64 cliques of 2^20..2^23
        // entries, cardinalities 2..16: message bytes / table bytes ~ 0.1-0.2 for branching cliques of
        // binary variables, 0.03-0.07 with wider ones; chains of any shape tested (cardinality 4..128)
        // were 1.2-1.7x faster traffic first.
        int policy = hp.layout_policy;
        if (policy == 0 && !seps.empty()) {
            double msg_bytes = 0;
            for (int sp : seps) {
                int sb = 0;
                for (int v : hp.ps[sp].vars) sb += hp.vbits[v];
                msg_bytes += 8.0 * (double)((int64_t)1 << sb);
            }
            if (wants_static(p)) {
                int sb = 0;
                for (int v : p.cover) sb += hp.vbits[v];
                msg_bytes += 8.0 * (double)((int64_t)1 << sb);
            }
            int cb = 0;
            for (int v : host) cb += hp.vbits[v];
            const double r = msg_bytes / ((double)((int64_t)1 << std::max(cb, hp.TB + JT_MIN_ITER_LOG2)) * esize);
            // (wide variables move the crossover down: the classes of policy 3 cannot split a variable)
            const double thr = (double)cb / std::max<size_t>(host.size(), 1) >= 2.0 ? 0.04 : 0.12;
            policy = (r >= thr || (p.children.size() <= 1 && r >= 0.01)) ? 2 : 3;
            // where the messages weigh that much: search the thread part with the cost model (multi-set plans keep
            // the heuristic: their sub-boxes have a hard per-set budget that the model does not know)
            if ((policy == 2 || hp.knobs.search_all) && !hp.multiset && !hp.knobs.no_search) policy = 4;
        }
        if (policy == 4 && (seps.empty() || !searched_order(c, host, seps, order))) policy = 2, order.clear();
        p.layout = policy;
        if (policy == 4) {
            // order filled by searched_order
        } else if (policy == 1 || seps.empty()) {
            order.assign(host.rbegin(), host.rend());
        } else if (policy == 2) {
            // Message traffic first (separators nearly as large as the cliques: every message entry is
            // used only a few times): variables in the fewest messages go lowest, so that the elements
            // one workgroup covers (thread part + loops) touch as few distinct entries of each message as
            // possible - a variable absent from a message costs that message's sub-box nothing.
            std::vector<std::pair<int, int>> keyed;           // (messages containing v, position in host order)
            for (size_t i = 0; i < host.size(); ++i) {
                int cnt = 0;
                for (int sp : seps) cnt += find_var(hp.ps[sp].vars, host[i]) >= 0;
                keyed.push_back({cnt, (int)i});
            }
            // (among variables of equally many messages, powers of two lowest: the thread part is the one place
            //  where a cardinality is still padded to a power of two)
            auto waste = [&](int i) { return (double)(1 << hp.vbits[host[i]]) / hp.card[host[i]]; };
            std::stable_sort(keyed.begin(), keyed.end(), [&](const std::pair<int, int> &a, const std::pair<int, int> &b) {
                return a.first != b.first ? a.first < b.first : waste(a.second) < waste(b.second);
            });
            // (moving variables of every message onto the wave bits, to spare the epilogues their barriers,
            //  was tried: the larger sub-boxes cost more than the barriers - config 3 27 -> 37 ms)
            for (auto &kv : keyed) order.push_back(host[kv.second]);
        } else {
            // Classes: priv = in no separator; ponly = only in the parent's; xorc = in some but not
            // all child separators; allc = in every child separator (leaf: in the parent's).
            // Target shape, low to high:  e bits <- priv | lane bits <- xorc | wave bits <- allc |
            // rest of xorc, allc | ponly, priv.  Bits of outgoing messages that sit in the thread
            // part need no cross-lane sum and no outer (A) loop; bits in every outgoing message can
            // be fixed per workgroup (F) without partial copies; everything else up high becomes the
            // register-summed R loop of the distribute pass, which moves twice the bytes of collect.
            int nchild = (int)p.children.size();
            std::vector<int> priv, ponly, part, allc;
            int n_full = 0;
            for (size_t i = 0; i < host.size(); ++i) {
                int v = host[i];
                int in_parent = p.psep >= 0 && find_var(hp.ps[p.psep].vars, v) >= 0;
                int in_child = 0;
                for (int k : p.children) in_child += find_var(hp.ps[hp.pn[k].psep].vars, v) >= 0;
                if (!in_parent && !in_child) priv.push_back(v);
                else if ((nchild > 0 && in_child == nchild) || nchild == 0) {
                    // variables of EVERY message (parent's too) first: they are never summed over in
                    // either pass, so they are the best occupants of the thread part
                    if (in_parent && nchild > 0) allc.insert(allc.begin() + n_full++, v);
                    else allc.push_back(v);
                } else if (in_child == 0) ponly.push_back(v);
                else part.push_back(v);
            }
            // (inside every class, powers of two first: they are the ones taken into the thread part, the one place
            //  where a cardinality is still padded to a power of two)
            for (std::vector<int> *cls : {&priv, &ponly, &part})
                std::stable_sort(cls->begin(), cls->end(), [&](int a, int b) {
                    return (double)(1 << hp.vbits[a]) / hp.card[a] < (double)(1 << hp.vbits[b]) / hp.card[b];
                });
            auto take = [&](std::vector<int> &from, int want_bits) {
                int got = 0;
                while (!from.empty() && got < want_bits) {
                    int v = from.front();
                    from.erase(from.begin());
                    order.push_back(v);
                    got += hp.vbits[v];
                }
                return got;
            };
            auto bits_of = [&](const std::vector<int> &l) {
                int b = 0;
                for (int v : l) b += hp.vbits[v];
                return b;
            };
            // (variables are not split: a wide variable taken for the element bits spills into the
            // lane bits, so without a private variable prefer one that outgoing messages contain)
            int got = take(priv, hp.EB);
            if (got < hp.EB) got += take(part, hp.EB - got);
            if (got < hp.EB) got += take(allc, hp.EB - got);
            if (got < hp.EB) got += take(ponly, hp.EB - got);
            int lane = got > hp.EB ? got - hp.EB : 0;       // bits a wide variable already spilled
            lane += take(part, 6 - std::min(lane, 6));
            // lanes prefer message bits (no shuffle sum) but leave two allc bits for the waves
            while (lane < 6 && !allc.empty() && bits_of(allc) - hp.vbits[allc.front()] >= 2) lane += take(allc, 1);
            if (lane < 6) lane += take(ponly, 6 - lane);
            if (lane < 6) lane += take(priv, 6 - lane);
            if (lane < 6) lane += take(allc, 6 - lane);
            int wave = take(allc, 2);
            if (wave < 2) wave += take(part, 2 - wave);
            if (wave < 2) wave += take(ponly, 2 - wave);
            if (wave < 2) wave += take(priv, 2 - wave);
            // Above the thread part: bits of no outgoing message first (they become the register-summed R
            // loop), bits of every child separator last (they become the chunk bits F), so that a workgroup's
            // loop rows are consecutive 4 KiB pieces of the table wherever the classes allow.  Rows strided
            // by 16-64 KiB stream 10-20 % slower than consecutive ones (tools/dma_bench.hip: 5.0 against
            // 6.2 TB/s read, 4.5 against 5.7 read+write); measured on C4: 1.5 %.
            take(priv, 1 << 20);
            take(ponly, 1 << 20);
            take(part, 1 << 20);
            take(allc, 1 << 20);
        }
        p.vars = order;
        p.pos.clear();
        p.nb.clear();
        // Thread part at true cardinalities (round 3): where a variable of the low TB index bits is not a power of two, those
        // variables become mixed-radix digits of a row of prod(card) elements instead of 2^TB - five variables of cardinality 3
        // in ten bits stored 4.2 x the table (round 2).  Such a clique keeps every variable wholly below or wholly above bit TB
        // (bits in between are padding: tpad_mask), and all tasks of the plan reach their elements through PNode::tmap.
        {
            // (Which cliques: those whose bit-field thread part would be filled to less than PlanKnobs::tmix_fill, 0.6 -
            //  cardinality 3: (3/4)^5 = 0.24, 5: 0.24, 6: 0.42.  Fuller ones keep the bit fields: a bit-field thread part may
            //  hold the low bit of one more variable, so it needs fewer rows - cardinality 7, width 7: fill 0.67, 0.30 ms
            //  against 0.46 ms with mixed-radix rows for 1.7 x the memory; tools/odd_time.py.)
            int b = 0;
            double fill = 1.0;
            for (int v : p.vars) {
                if (b + hp.vbits[v] <= hp.TB) fill *= (double)hp.card[v] / (double)(1 << hp.vbits[v]);
                b += hp.vbits[v];
            }
            // (a unit clique stores nothing: no rows to pack - it keeps the bit-field thread part, whose entries that name
            //  no table entry its thread map marks)
            p.tmix = fill < hp.knobs.tmix_fill && hp.compact && !hp.multiset && !hp.knobs.no_tmix && !p.unit;
        }
        int bit = 0;
        p.tpad_mask = 0;
        p.tsplit = -1, p.tsplit_lb = 0;
        for (int v : p.vars) {
            if (p.tmix && bit < hp.TB && bit + hp.vbits[v] > hp.TB) {
                // A variable across bit TB: its low bits become a radix-2^lb digit of the row and its high bits a digit of the rows
                // above with ceil(card / 2^lb) values - the rows of a bit-field thread part, a third to a half fewer than with the
                // variable moved up whole - where the entries this stores for values >= card (zeros) cost at most a quarter;
                // else the variable moves above bit TB and the bits below it are padding.
                const int lb = hp.TB - bit, card = hp.card[v], hi = (card + (1 << lb) - 1) >> lb;
                if (!hp.knobs.no_tsplit && (double)(hi << lb) <= 1.25 * card) {
                    p.tsplit = (int)p.pos.size(), p.tsplit_lb = lb;
                } else {
                    for (int b = bit; b < hp.TB; ++b) p.tpad_mask |= 1u << b;
                    bit = hp.TB;
                }
            }
            if (p.unit && bit < hp.TB && bit + hp.vbits[v] > hp.TB && (hp.card[v] & (hp.card[v] - 1)) != 0) {
                // A unit clique has no table whose zeros could mark the entries that do not exist: which entries of a ROW exist must
                // depend on the thread alone (PNode::tmap) and which rows exist on the row alone (JT_NO_ROW).  A variable across bit
                // TB whose cardinality is no power of two would tie the two together: it moves above bit TB whole.
                for (int b = bit; b < hp.TB; ++b) p.tpad_mask |= 1u << b;
                bit = hp.TB;
            }
            p.pos.push_back(bit);
            p.nb.push_back(hp.vbits[v]);
            bit += hp.vbits[v];
        }
        if (p.tmix || p.unit)
            for (int b = bit; b < hp.TB; ++b) p.tpad_mask |= 1u << b;
        hp.tmix = hp.tmix || p.tmix;
        if (bit > JT_MAX_BITS) FAIL(JTP_EUNSUPPORTED, "clique %d needs %d index bits (max %d)", p.real, bit, JT_MAX_BITS);
        p.nbits = std::max(bit, hp.TB + JT_MIN_ITER_LOG2);   // >= 4 loop iterations per workgroup
        if (p.nbits - hp.TB > JT_MAX_HI) FAIL(JTP_EUNSUPPORTED, "clique %d too large", p.real);
        // Physical layout (jtp_internal.h, JT_NO_ROW): rows above the thread part.  A variable that starts inside
        // the thread part keeps its bit field (its upper bits double the row stride); a variable wholly above it
        // whose cardinality is not a power of two is stored at its true cardinality - its bits form a group that
        // every task keeps together; index bits above the last variable are padding and store nothing.
        p.bitw.assign(p.nbits, 0);
        p.group_mask.clear();
        p.group_pos.clear();
        p.group_card.clear();
        p.pad_mask = 0;
        for (int b = 0; b < hp.TB && b < p.nbits; ++b) p.bitw[b] = (int64_t)1 << b;
        int64_t mult = (int64_t)1 << hp.TB;
        p.trow = 1 << hp.TB;
        p.tmap.clear();
        if (p.tmix) {
            // row = the thread-part variables as mixed-radix digits, first variable fastest
            std::vector<int64_t> tstride(p.vars.size(), 0);
            int64_t prod = 1;
            for (size_t i = 0; i < p.vars.size(); ++i) {
                if (p.pos[i] + p.nb[i] <= hp.TB) tstride[i] = prod, prod *= hp.card[p.vars[i]];
                else if ((int)i == p.tsplit) tstride[i] = prod, prod <<= p.tsplit_lb;          // the low bits of the variable across TB
            }
            p.trow = (int)((prod + hp.VEC - 1) / hp.VEC * hp.VEC);
            p.tmap.assign((size_t)1 << hp.TB, -1);
            for (uint32_t x = 0; x < (1u << hp.TB); ++x) {
                if (x & p.tpad_mask) continue;
                int64_t off = 0;
                bool ok = true;
                for (size_t i = 0; i < p.vars.size() && ok; ++i) {
                    if ((int)i == p.tsplit) {
                        off += (int64_t)((x >> p.pos[i]) & ((1u << p.tsplit_lb) - 1u)) * tstride[i];       // (every low value has a place)
                        continue;
                    }
                    if (p.pos[i] + p.nb[i] > hp.TB) continue;
                    const int digit = (int)((x >> p.pos[i]) & ((1u << p.nb[i]) - 1u));
                    ok = digit < hp.card[p.vars[i]];
                    off += digit * tstride[i];
                }
                if (ok) p.tmap[x] = (int32_t)off;
            }
            for (int b = 0; b < hp.TB && b < p.nbits; ++b) p.bitw[b] = 0;      // (inside a row: tmap, not bit weights)
            mult = p.trow;
            // compact form (round 5): the logical threads that own an entry, if two waves hold them all
            p.vmap.clear();
            if (!hp.multiset && !hp.knobs.no_vgroups && !p.unit) {
                std::vector<int32_t> owners;
                int spare = -1;
                for (int t = 0; t < JT_THREADS; ++t) {
                    bool any = false;
                    for (int e = 0; e < hp.VEC; ++e) any = any || p.tmap[(size_t)t * hp.VEC + e] >= 0;
                    if (any) owners.push_back(t);
                    else if (spare < 0) spare = t;
                }
                if (owners.size() <= 128 && (owners.size() == 128 || spare >= 0)) {
                    p.vmap = owners;
                    p.vmap.resize(128, spare);
                }
            }
        }
        for (size_t i = 0; i < p.vars.size(); ++i) {
            const int pos = p.pos[i], nb = p.nb[i], card = hp.card[p.vars[i]];
            if (pos + nb <= hp.TB) continue;
            // (a unit clique has no table whose zeros could stand for a digit beyond the cardinality: its rows are always counted at
            //  the true cardinalities, JTP_NO_COMPACT or not)
            const bool whole = pos >= hp.TB && (hp.compact || p.unit) && (card & (card - 1)) != 0;
            // (the variable across TB of a mixed-radix clique: its high bits are a digit of ceil(card / 2^lb) values)
            const int hi = (int)i == p.tsplit ? (card + (1 << p.tsplit_lb) - 1) >> p.tsplit_lb : 0;
            const bool split_group = hi > 0 && (hi & (hi - 1)) != 0;
            for (int k = std::max(0, hp.TB - pos); k < nb; ++k) {
                p.bitw[pos + k] = whole ? mult << k : (split_group ? mult << (k - (hp.TB - pos)) : mult);
                if (!whole && !split_group) mult <<= 1;
            }
            if (whole) {
                p.group_mask.push_back(((1u << nb) - 1u) << pos);
                p.group_pos.push_back(pos);
                p.group_card.push_back(card);
                mult *= card;
            } else if (split_group) {
                p.group_mask.push_back(((1u << (nb - (hp.TB - pos))) - 1u) << hp.TB);
                p.group_pos.push_back(hp.TB);
                p.group_card.push_back(hi);
                mult *= hi;
            }
        }
        for (int b = std::max(bit, hp.TB); b < p.nbits; ++b) {
            if (hp.compact || p.unit) p.pad_mask |= 1u << b; // weight 0, exists only when clear
            else p.bitw[b] = mult, mult <<= 1;
        }
        p.phys_elems = mult;
        if (mult > ((int64_t)1 << 31)) FAIL(JTP_EUNSUPPORTED, "clique %d too large", p.real);
    }
    for (PNode &p : hp.pn)
        if (!p.tmix && (hp.tmix || p.unit)) {
            // bit-field rows: the identity map, so that one kernel family serves every task of a plan with mixed-radix rows; a unit
            // clique's map says which entries of a row EXIST (-1: a thread-part variable's digit beyond its cardinality, an index bit
            // below TB that no variable owns) - the zeros a stored table would hold there
            p.tmap.resize((size_t)1 << hp.TB);
            for (uint32_t x = 0; x < (1u << hp.TB); ++x) {
                bool ok = true;
                if (p.unit) {
                    ok = !(x & p.tpad_mask);
                    for (size_t i = 0; i < p.vars.size() && ok; ++i)
                        if (p.pos[i] + p.nb[i] <= hp.TB) ok = (int)((x >> p.pos[i]) & ((1u << p.nb[i]) - 1u)) < hp.card[p.vars[i]];
                }
                p.tmap[x] = ok ? (int32_t)x : -1;
            }
        }
    for (size_t s = 0; s < hp.ps.size(); ++s) {
        PSep &sp = hp.ps[s];
        const PNode &ch = hp.pn[sp.child];
        std::vector<int> order;
        for (int v : ch.vars)
            if (find_var(sp.vars, v) >= 0) order.push_back(v);
        sp.vars = order;
        int bit = 0;
        sp.pos.clear();
        sp.nb.clear();
        for (int v : sp.vars) {
            sp.pos.push_back(bit);
            sp.nb.push_back(hp.vbits[v]);
            bit += hp.vbits[v];
        }
        sp.nbits = bit;
        if (bit > 28) FAIL(JTP_EUNSUPPORTED, "separator with %d index bits", bit);
    }
    // static tables of unit cliques: the covered variables in the clique's device order, a plain bit field like a message
    for (int c = 0; c < NP; ++c) {
        PNode &p = hp.pn[c];
        if (!wants_static(p)) continue;
        PStatic st;
        st.pnode = c;
        int bit = 0;
        for (int v : p.vars)
            if (find_var(p.cover, v) >= 0) {
                st.vars.push_back(v);
                st.pos.push_back(bit);
                st.nb.push_back(hp.vbits[v]);
                bit += hp.vbits[v];
            }
        st.nbits = bit;
        if (bit > 28) FAIL(JTP_EUNSUPPORTED, "static table with %d index bits", bit);
        p.stat = (int)hp.statics.size();
        hp.statics.push_back(st);
    }

    return JTP_OK;
}
