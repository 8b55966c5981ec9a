// Instrumentation: profiling events of the propagate, timed regions, plan statistics, a debugging view of the message arena.
// Launches nothing: host code over the HIP runtime.
#include <algorithm>
#include <cstring>

#include "jtp_engine.h"

extern "C" {

int jtp_set_profiling(jtp_plan *pl, int32_t on) {
    if (!pl) return set_err(JTP_EINVAL, "null plan");
    pl->prof_steps = on > 0 ? std::min(on, 256) : 0;     // `on` = number of propagates to keep
    pl->prof_cursor = 0;
    pl->prof_calls = 0;
    return JTP_OK;
}

int jtp_set_profiling_stride(jtp_plan *pl, int32_t stride) {
    if (!pl) return set_err(JTP_EINVAL, "null plan");
    if (stride < 1) return set_err(JTP_EINVAL, "stride must be at least 1");
    pl->prof_stride = stride;
    pl->prof_calls = 0;
    pl->prof_cursor = 0;
    return JTP_OK;
}

int jtp_set_profiling_granularity(jtp_plan *pl, int32_t per_launch) {
    if (!pl) return set_err(JTP_EINVAL, "null plan");
    pl->prof_per_launch = per_launch != 0;
    pl->prof_cursor = 0;
    return JTP_OK;
}

// ONE event pair around a whole region of propagates (a benchmark's timed steps): the device time from the first launch of
// the region to the end of its last, nothing in between - per-propagate events cost 2-3 us of idle GPU each, and a span
// that contains them reads longer than the step it is meant to time.
int jtp_region_begin(jtp_plan *pl) {
    int rc = check_ready(pl, 0);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(pl->hp.device));
    for (int i = 0; i < 2; ++i)
        if (!pl->region_ev[i]) HIP_TRY(hipEventCreate(&pl->region_ev[i]));
    HIP_TRY(hipEventRecord(pl->region_ev[0], pl->streams[0]));
    pl->region_open = true;
    return JTP_OK;
}

int jtp_region_end(jtp_plan *pl, double *ms) {
    int rc = check_ready(pl, 0);
    if (rc) return rc;
    if (!pl->region_open || !ms) return set_err(JTP_EINVAL, "jtp_region_end without jtp_region_begin");
    HIP_TRY(hipSetDevice(pl->hp.device));
    HIP_TRY(hipEventRecord(pl->region_ev[1], pl->streams[0]));
    HIP_TRY(hipEventSynchronize(pl->region_ev[1]));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, pl->region_ev[0], pl->region_ev[1]));
    *ms = t;
    pl->region_open = false;
    return JTP_OK;
}

int jtp_get_stats(jtp_plan *pl, jtp_stats *st) {
    if (!pl || !st) return set_err(JTP_EINVAL, "null argument");
    HostPlan &hp = pl->hp;
    memset(st, 0, sizeof *st);
    st->struct_size = (int32_t)sizeof(jtp_stats);
    const bool flow = pl->flow && !pl->prof_per_launch;
    st->n_launches = (int32_t)(flow ? hp.segments.size() : hp.launches.size());
    for (const Step &sp : hp.steps) st->n_launches += sp.kind == 2 ? 1 : 0;      // (JTP_SCALED: the rescale launches between the levels)
    st->n_messages = hp.n_messages;
    st->n_tasks = (int32_t)hp.tasks.size();
    // multi-set plans: a table is read once per GROUP of evidence sets, messages once per set
    st->algorithmic_bytes = hp.alg_bytes;
    if (pl->multiset) {
        // what THIS engine streams: a table once per pass and GROUP of evidence sets that runs the pass (group 0 - the evidence-free
        // sets - included; a (task, group) whose subtree meets no evidence copies group 0's message and streams nothing), messages per set
        double tb = 0;
        for (const Launch &L : hp.launches) {
            if (L.variant != JT_K_MULTI_COLLECT && L.variant != JT_K_MULTI_DISTRIBUTE) continue;
            for (int t : L.tasks) {
                const PNode &p = hp.pn[hp.tasks[t].pnode];
                const double table = hp.tasks[t].kind == 0 && p.real >= 0 ? (double)hp.pack[p.real].host_elems * pl->esize : 0.0;
                tb += table * (pl->act_n_host.empty() ? pl->n_groups : (pl->act_n_host[t] + JT_MSETS - 1) / JT_MSETS);
            }
        }
        st->algorithmic_bytes = tb + hp.alg_msg_bytes * hp.n_batch;
    }
    st->flow_fallbacks = pl->flow_fallbacks;
    st->launch_mode = pl->launch_mode;
    st->tickets_used = pl->tickets_used;
    st->flow_propagates = pl->flow_propagates;
    st->device_bytes = pl->device_bytes;
    st->storage_dtype = hp.dtype;
    st->foreign_seen = pl->foreign_seen;
    st->flight_board = flight_board_state(hp.device);
    st->algorithmic_bytes_full = hp.alg_bytes_full;
    st->fixed_bytes = (double)hp.fix_doubles * 8;
    st->lean_refused = hp.lean_refused.empty() ? 0 : 1;
    for (int c = 0; c < hp.n_cliques; ++c) {
        st->n_unit_cliques += hp.pn[c].unit ? 1 : 0;
        st->n_static_tables += hp.pn[c].unit && hp.pn[c].stat >= 0 ? 1 : 0;
    }
    if (pl->multiset) {
        const int groups = pl->n_groups;
        // float64 operations of the element loop of jt_mpass, per thread and table row (VEC elements), G = JT_MSETS sets:
        //   elements summed first (JtTask::esum == 3): VEC - 1 additions, then per set (n_in - 1) multiplications and one
        //   fused multiply-add;  no message on the element bits: per set (n_in - 1) multiplications and VEC fused multiply-adds;
        //   else per set and element n_in multiplications and one fused multiply-add
        const int VEC = hp.VEC;
        double flops = 0, insts = 0;
        for (const Launch &L : hp.launches) {
            if (L.variant != JT_K_MULTI_COLLECT && L.variant != JT_K_MULTI_DISTRIBUTE) continue;
            for (int t : L.tasks) {
                const JtTask &tk = hp.tasks[t];
                if (tk.kind != 0) continue;
                bool edep = false;
                for (int k = 0; k < tk.n_in; ++k) edep = edep || tk.msg[k].e_dep != 0;
                const double nin1 = std::max(tk.n_in - 1, 0);
                const double rows = (double)JT_THREADS * (double)tk.total * (double)(1u << tk.nF);
                const int runs = pl->act_n_host.empty() ? pl->n_groups : (pl->act_n_host[t] + JT_MSETS - 1) / JT_MSETS;
                for (int g = 0; g < runs; ++g) {
                    double per, ins;
                    const bool sum_first = pl->act_n_host.empty() ? ((tk.esum_groups >> (g & 63)) & 1ull) != 0 : pl->esum_oct_host[(size_t)t * pl->n_groups + g] != 0;
                    if ((tk.esum & 1) && sum_first && tk.setb <= JT_SETB_SMALL)
                        per = (VEC - 1) + JT_MSETS * (nin1 + 2.0), ins = (VEC - 1) + JT_MSETS * (nin1 + 1.0);
                    else if (!edep) per = JT_MSETS * (nin1 + 2.0 * VEC), ins = JT_MSETS * (nin1 + VEC);
                    else per = JT_MSETS * VEC * (tk.n_in + 2.0), ins = JT_MSETS * VEC * (tk.n_in + 1.0);
                    flops += per * rows;
                    insts += ins * rows;
                }
            }
        }
        st->f64_flops = flops;
        st->f64_insts = insts;
        for (const Launch &L : hp.launches) {
            if (L.variant != JT_K_MULTI_COLLECT && L.variant != JT_K_MULTI_DISTRIBUTE) continue;
            double tb = 0, mb = 0;
            for (int t : L.tasks) {
                const PNode &p = hp.pn[hp.tasks[t].pnode];
                const double table = p.real >= 0 ? (double)hp.pack[p.real].host_elems * pl->esize : 0.0;
                tb += table;
            }
            mb = L.alg_bytes - tb;
            st->kernel_bytes[L.variant] += tb * groups + mb * hp.n_batch;
        }
        for (const Segment &sg : hp.segments) st->kernel_launches[sg.phase == 0 ? JT_K_MULTI_COLLECT : JT_K_MULTI_DISTRIBUTE] += flow ? 1 : sg.n_launch;
    } else if (flow) {
        for (const Segment &sg : hp.segments) {
            // (the kernel that actually runs: KernelTable::get_flow)
            const int v = sg.phase == 0 ? JT_K_COLLECT_FLOW : (sg.phase == 1 && (pl->chain || hp.tmix || !flow_both()) ? JT_K_DISTRIBUTE_FLOW : JT_K_BOTH_FLOW);
            for (int i = sg.first_launch; i < sg.first_launch + sg.n_launch; ++i) st->kernel_bytes[v] += hp.launches[i].alg_bytes;
            st->kernel_launches[v] += 1;
        }
    } else {
        for (size_t i = 0; i < hp.launches.size(); ++i) {
            const Launch &L = hp.launches[i];
            st->kernel_bytes[L.variant] += L.alg_bytes;
            st->kernel_launches[L.variant] += 1;
        }
    }
    if (pl->device && pl->prof_steps > 0 && pl->prof_cursor > 0) {
        HIP_TRY(hipSetDevice(hp.device));
        const int kept = std::min(pl->prof_cursor, pl->prof_steps);
        if (pl->prof_per_launch) {
            for (int k = 0; k < kept; ++k) {
                const size_t base = 2 * hp.launches.size() * (size_t)k;
                for (size_t i = 0; i < hp.launches.size(); ++i) {
                    const Launch &L = hp.launches[i];
                    HIP_TRY(hipEventSynchronize(pl->ev[base + 2 * i + 1]));
                    float ms = 0;
                    HIP_TRY(hipEventElapsedTime(&ms, pl->ev[base + 2 * i], pl->ev[base + 2 * i + 1]));
                    st->kernel_ms[L.variant] += ms / kept;      // mean per propagate
                    if (L.phase == 0) st->collect_ms += ms / kept;
                    else st->distribute_ms += ms / kept;
                }
            }
        } else {
            for (int k = 0; k < kept; ++k) {
                const size_t base = 3 * (size_t)k;
                HIP_TRY(hipEventSynchronize(pl->ev[base + 2]));
                float c = 0, d = 0;
                HIP_TRY(hipEventElapsedTime(&c, pl->ev[base + 0], pl->ev[base + 1]));
                HIP_TRY(hipEventElapsedTime(&d, pl->ev[base + 1], pl->ev[base + 2]));
                st->collect_ms += c / kept;
                st->distribute_ms += d / kept;
            }
            // with one kernel per phase (the default), the phase time is that kernel's time over
            // its back-to-back launches (gaps included)
            if (pl->multiset) {
                st->kernel_ms[JT_K_MULTI_COLLECT] = st->collect_ms;
                st->kernel_ms[JT_K_MULTI_DISTRIBUTE] = st->distribute_ms;
            } else if (flow) {
                bool merged = false;
                for (const Segment &sg : hp.segments) merged = merged || sg.phase == 2;
                if (merged && hp.segments.size() == 1) {
                    st->kernel_ms[JT_K_BOTH_FLOW] = st->collect_ms + st->distribute_ms;       // one launch: the whole propagate
                } else if (merged) {
                    // (sharded plans: a collect launch, the exchange, then the merged launch)
                    st->kernel_ms[JT_K_COLLECT_FLOW] = st->collect_ms;
                    st->kernel_ms[JT_K_BOTH_FLOW] = st->distribute_ms;
                } else {
                    st->kernel_ms[JT_K_COLLECT_FLOW] = st->collect_ms;
                    st->kernel_ms[(pl->chain || hp.tmix || !flow_both()) ? JT_K_DISTRIBUTE_FLOW : JT_K_BOTH_FLOW] = st->distribute_ms;
                }
            } else if (!(hp.flags & JTP_SPLIT_VARIANTS)) {
                st->kernel_ms[JT_K_COLLECT_LEVEL] = st->collect_ms;
                st->kernel_ms[JT_K_DISTRIBUTE_LEVEL] = st->distribute_ms;
            }
        }
    }
    return JTP_OK;
}

int jtp_debug_read_msg(jtp_plan *pl, int32_t batch, int64_t off, int64_t n, double *host) {
    int rc = check_ready(pl, batch);
    if (rc) return rc;
    if (off < 0 || n < 0 || off + n > pl->hp.msg_doubles) return set_err(JTP_EINVAL, "range outside the message arena");
    HIP_TRY(hipSetDevice(pl->hp.device));
    HIP_TRY(hipMemcpy(host, pl->bufs[batch].msg + off, (size_t)n * 8, hipMemcpyDeviceToHost));
    return JTP_OK;
}

int jtp_get_launch_ms(jtp_plan *pl, double *out, int32_t n) {
    if (!pl) return set_err(JTP_EINVAL, "null plan");
    HostPlan &hp = pl->hp;
    const int nl = (int)hp.launches.size();
    if (!(pl->device && pl->prof_steps > 0 && pl->prof_cursor > 0 && pl->prof_per_launch))
        return set_err(JTP_EINVAL, "per-launch profiling is off or nothing was recorded");
    HIP_TRY(hipSetDevice(hp.device));
    const int kept = std::min(pl->prof_cursor, pl->prof_steps);
    for (int i = 0; i < nl && i < n; ++i) out[i] = 0.0;
    for (int k = 0; k < kept; ++k) {
        const size_t base = 2 * hp.launches.size() * (size_t)k;
        for (int i = 0; i < nl && i < n; ++i) {
            HIP_TRY(hipEventSynchronize(pl->ev[base + 2 * i + 1]));
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, pl->ev[base + 2 * i], pl->ev[base + 2 * i + 1]));
            out[i] += ms / kept;
        }
    }
    return nl;
}

}  // extern "C"
