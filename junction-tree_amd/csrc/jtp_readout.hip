// Data out: beliefs of cliques and separators, marginals over request lists (kept with the plan), the scale of JTP_SCALED
// plans with Z and log Z, and expected counts over evidence sets.  Off the hot path, except where a model reads marginals per step.
#include <cmath>

#include <algorithm>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "jtp_engine.h"

// ------------------------------------------------------------------------------------------ kernels

// host index -> device index
__device__ __forceinline__ uint32_t jt_host_to_dev(const JtPackDesc &d, int64_t h) {
    uint32_t x = 0;
    for (int i = d.nvars - 1; i >= 0; --i) {
        const int c = d.card[i];
        const int digit = (int)(h % c);
        h /= c;
        if (d.row_elems > 0 && i == d.split_var)
            x += (uint32_t)(digit & ((1 << d.split_lb) - 1)) * d.dstride[i] + (uint32_t)(digit >> d.split_lb) * d.split_ds2;
        else
        x += (uint32_t)digit * d.dstride[i];
    }
    return x;
}

template <typename T, typename S>
__global__ __launch_bounds__(256) void jt_unpack(JtPackDesc d, const T *__restrict__ arena, S *__restrict__ stage) {
    for (int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; h < d.host_elems;
         h += (int64_t)gridDim.x * blockDim.x)
        stage[h] = (S)arena[d.dev_off + jt_host_to_dev(d, h)];
}

// message(s) -> host order: out[h] = (sum_p up[p]) * (dn ? sum_p dn[p] : 1)
template <typename S>
__global__ __launch_bounds__(256) void jt_msg_unpack(JtPackDesc d, const double *__restrict__ up, int up_npart,
                                                     const double *__restrict__ dn, int dn_npart, int64_t pstride,
                                                     S *__restrict__ stage) {
    for (int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; h < d.host_elems;
         h += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t x = jt_host_to_dev(d, h);
        double u = 0.0;
        for (int p = 0; p < up_npart; ++p) u += up[(int64_t)p * pstride + x];
        if (dn) {
            double w = 0.0;
            for (int p = 0; p < dn_npart; ++p) w += dn[(int64_t)p * pstride + x];
            u *= w;
        }
        stage[h] = (S)u;
    }
}

// batched marginal read-out: request blockIdx.y, entries strided over blockIdx.x
// (round 6: a factor marginal is a few dozen entries of hundreds of partial copies - one per workgroup of the pass that formed it; a
//  thread per entry added them one after the other, 94 us for config 3's 1831 requests.  A request of at most 128 entries now spreads
//  its copies over 256 / entries thread groups - group g takes copies g, g + G, ... - whose sums are added in group order: a fixed
//  order, the same bits on every call.)
__global__ __launch_bounds__(256) void jt_marg_unpack(const JtMargDesc *__restrict__ descs, const double *__restrict__ scratch_buf,
                                                      double *__restrict__ stage, const double *__restrict__ arena_cur) {
    const JtMargDesc &m = descs[blockIdx.y];
    const double *scratch = m.in_arena ? arena_cur : scratch_buf;       // (a marginal a folded task left in the message arena)
    __shared__ double part[256];
    const int64_t ne = m.d.host_elems;
    if (ne <= 128 && gridDim.x == 1) {
        int w = 1;
        while (w < ne) w <<= 1;                                   // entries rounded up to a power of two
        const int G = 256 / w, g = (int)threadIdx.x / w, h = (int)threadIdx.x % w;
        double u = 0.0;
        if (h < ne) {
            const uint32_t x = jt_host_to_dev(m.d, h);
            for (int p = g; p < m.npart; p += G) u += scratch[m.src_off + (int64_t)p * m.pstride + x];
        }
        part[threadIdx.x] = u;
        __syncthreads();
        if (g == 0 && h < ne) {
            double t = part[h];
            for (int k = 1; k < G; ++k) t += part[k * w + h];
            stage[m.dst_off + h] = t;
        }
        return;
    }
    for (int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; h < ne; h += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t x = jt_host_to_dev(m.d, h);
        double u = 0.0;
        for (int p = 0; p < m.npart; ++p) u += scratch[m.src_off + (int64_t)p * m.pstride + x];
        stage[m.dst_off + h] = u;
    }
}

// Expected counts (jtp_accumulate_marginals): the scratch buffer holds one slot per evidence set of a chunk, `slot_stride` doubles
// apart, each laid out as the request list's own (JtMargDesc::src_off).
//
// jt_marg_sums, a workgroup per (request blockIdx.x, slot blockIdx.y): the entries of the request - its partial copies added up - go
// to `entries` (per slot the layout of the read-out's staging buffer, `out_stride` doubles apart), their sum S to `sums`.  Copies
// are added as jt_marg_unpack adds them: a request of at most 128 entries spreads them over 256 / entries thread groups (group g
// takes copies g, g + G, ... in ascending order, the groups' sums are added in group order), a larger one adds them in ascending
// order, a thread per entry.  S: thread t adds entries t, t + 256, ... in that order, the 256 partial sums go through a fixed halving
// tree.  The order of every addition depends on the request's entry and copy counts alone.  The last request of the list is the root's
// scalar: its S is also the set's root sum (`roots`, one per slot).
__global__ __launch_bounds__(256) void jt_marg_sums(const JtMargDesc *__restrict__ descs, const double *__restrict__ scratch, int64_t slot_stride,
                                                    int n_all, double *__restrict__ entries, int64_t out_stride, double *__restrict__ sums,
                                                    double *__restrict__ roots) {
    const JtMargDesc &m = descs[blockIdx.x];
    const double *sc = scratch + (int64_t)blockIdx.y * slot_stride + m.src_off;
    double *out = entries + (int64_t)blockIdx.y * out_stride + m.dst_off;
    __shared__ double part[256];
    const int tid = (int)threadIdx.x;
    const int64_t ne = m.d.host_elems;
    double t = 0.0;
    if (ne <= 128) {
        int w = 1;
        while (w < ne) w <<= 1;                                   // entries rounded up to a power of two
        const int G = 256 / w, g = tid / w, h = tid % w;
        double u = 0.0;
        if (h < ne) {
            const uint32_t x = jt_host_to_dev(m.d, h);
            for (int p = g; p < m.npart; p += G) u += sc[(int64_t)p * m.pstride + x];
        }
        part[tid] = u;
        __syncthreads();
        if (g == 0 && h < ne) {
            t = part[h];
            for (int k = 1; k < G; ++k) t += part[k * w + h];
            out[h] = t;
        }
        __syncthreads();
    } else {
        for (int64_t h = tid; h < ne; h += 256) {
            const uint32_t x = jt_host_to_dev(m.d, h);
            double u = 0.0;
            for (int p = 0; p < m.npart; ++p) u += sc[(int64_t)p * m.pstride + x];
            out[h] = u;
            t += u;
        }
    }
    part[tid] = t;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) part[tid] += part[tid + w];
        __syncthreads();
    }
    if (tid == 0) {
        sums[(int64_t)blockIdx.y * n_all + blockIdx.x] = part[0];
        if ((int)blockIdx.x == n_all - 1) roots[blockIdx.y] = part[0];
    }
}

// acc[entry] += w_b * (u_b / S_b) over the slots of the chunk in ascending order - one thread owns an entry for the whole call, so
// the additions into it come in the order of the evidence sets whatever the chunk size (no float atomics).  A set of weight 0 is
// skipped unread; a pair (set, request) whose S is zero or not finite contributes nothing and is reported: `bad[0]` counts the
// pairs, `bad[1]` keeps the smallest (set of the range) * n_all + request - integer atomics, whose result no order changes.
// Request blockIdx.x, entries strided over blockIdx.y; `weights` null: all 1; `first_set`: the chunk's first set within the range.
__global__ __launch_bounds__(256) void jt_marg_accumulate(const JtMargDesc *__restrict__ descs, const double *__restrict__ entries, int64_t out_stride,
                                                          int n_all, const double *__restrict__ sums, const double *__restrict__ weights, int n_slots,
                                                          int64_t first_set, double *__restrict__ acc, unsigned long long *__restrict__ bad) {
    const JtMargDesc &m = descs[blockIdx.x];
    if (blockIdx.y == 0 && threadIdx.x == 0)
        for (int k = 0; k < n_slots; ++k) {
            const double s = sums[(int64_t)k * n_all + blockIdx.x];
            if ((weights ? weights[k] : 1.0) != 0.0 && !(s != 0.0 && isfinite(s))) {
                atomicAdd(bad, 1ull);
                atomicMin(bad + 1, (unsigned long long)(first_set + k) * (unsigned long long)n_all + blockIdx.x);
            }
        }
    for (int64_t h = (int64_t)blockIdx.y * 256 + threadIdx.x; h < m.d.host_elems; h += (int64_t)gridDim.y * 256) {
        double a = acc[m.dst_off + h];
        for (int k = 0; k < n_slots; ++k) {
            const double w = weights ? weights[k] : 1.0, s = sums[(int64_t)k * n_all + blockIdx.x];
            if (w == 0.0 || !(s != 0.0 && isfinite(s))) continue;
            a += w * (entries[(int64_t)k * out_stride + m.dst_off + h] / s);
        }
        acc[m.dst_off + h] = a;
    }
}

// ------------------------------------------------------------------------------------------ helpers

// messages and marginals are plain bit fields of `nbits` bits: the layout record of one over `vars` (host axis order), variable i
// at bit pos[i], nb[i] bits wide
static JtPackDesc bitfield_desc(const HostPlan &hp, const std::vector<int> &vars, const int *pos, const int *nb, int nbits) {
    JtPackDesc d;
    memset(&d, 0, sizeof d);
    d.nvars = (int)vars.size();
    d.nbits = nbits;
    int64_t stride = 1;
    for (int i = d.nvars - 1; i >= 0; --i) {
        d.pos[i] = (uint8_t)pos[i];
        d.nb[i] = (uint8_t)nb[i];
        d.card[i] = hp.card[vars[i]];
        d.hstride[i] = stride;
        stride *= hp.card[vars[i]];
        d.dstride[i] = 1u << d.pos[i];
        d.dmod[i] = 1 << d.nb[i];
    }
    d.host_elems = stride;
    d.phys_elems = (int64_t)1 << d.nbits;
    d.low_bits = d.nbits;
    d.row_elems = 0;
    d.split_var = -1;
    return d;
}

// Multi-set plans with active lists (rebuild_active): the upward message of a (collect task, arena slot) that is NOT on the task's list
// exists in slot 0's arena only - nobody copies it into the set's own (round 5 did, after every propagate: 7 % of a 64-set step).  A
// read-out task of evidence set `batch` takes its inputs from that set's arena; an input formed by such a task has its offset moved
// back by the slot's distance, i.e. is read from slot 0.  `member_host` describes the lists the LAST propagate ran with.
static bool readout_redirect(const jtp_plan *pl, int batch, JtTask &tk) {
    if (!pl->multiset || pl->set0 == 0 || pl->member_host.empty()) return false;
    const size_t cap = (size_t)pl->n_groups * JT_MSETS, slot = (size_t)(pl->set0 + batch);
    bool any = false;
    for (int k = 0; k < tk.n_in; ++k) {
        const int t = tk.msg[k].src_task;
        if (t >= 0 && !pl->member_host[(size_t)t * cap + slot]) tk.msg[k].off -= (int64_t)slot * pl->set_stride, any = true;
    }
    return any;
}

// The JtFlow of a read-out launch: nobody waits on markers and the other arena half is left alone - so no abort flag, and none of
// JTP_FLOW_DEBUG's fault injection, which is the propagate's ...
static JtFlow readout_flow() {
    JtFlow fl;
    memset(&fl, 0, sizeof fl);
    fl.oth_off = -1;
    return fl;
}
// ... and, where its tasks take their inputs from the messages of the last propagate of evidence set `b`, where those are
static void readout_inputs(JtFlow &fl, const jtp_plan *pl, const BatchBuffers &b) {
    fl.cur_off = cur_half(pl, b);
    fl.ev = b.ev_any || pl->multiset ? b.ev : nullptr;
    fl.fix_shift = b.fix_shift(fl.cur_off);
}

// the key a list of marginal requests is kept under: n, cliques, offsets, variables
static std::vector<int32_t> marg_key(int32_t n, const int32_t *cliques, const int32_t *var_off, const int32_t *var_ids) {
    std::vector<int32_t> key;
    key.push_back(n);
    key.insert(key.end(), cliques, cliques + n);
    for (int i = 0; i <= n; ++i) key.push_back(var_off[i] - var_off[0]);
    key.insert(key.end(), var_ids + var_off[0], var_ids + var_off[n]);
    return key;
}

static MargBatch *find_marg_batch(jtp_plan *pl, const std::vector<int32_t> &key) {
    for (size_t i = 0; i < pl->marg_cache.size(); ++i)
        if (pl->marg_cache[i]->key == key) {                // most recently used last
            std::rotate(pl->marg_cache.begin() + i, pl->marg_cache.begin() + i + 1, pl->marg_cache.end());
            return pl->marg_cache.back().get();
        }
    return nullptr;
}

static MargBatch *keep_marg_batch(jtp_plan *pl, std::unique_ptr<MargBatch> &made) {
    if (pl->marg_cache.size() >= 32) pl->marg_cache.erase(pl->marg_cache.begin());      // a model asks for a few lists (and Z); keep the last used
    pl->marg_cache.push_back(std::move(made));
    return pl->marg_cache.back().get();
}

// The device tables of a request list that is not in the plan's cache yet, complete in `made` or not there at all: the plan
// itself is not touched (keep_marg_batch hands the list over).
static int make_marg_batch(jtp_plan *pl, const std::vector<int32_t> &key, int32_t n, const int32_t *cliques, const int32_t *var_off,
                           const int32_t *var_ids, std::unique_ptr<MargBatch> &made) {
    HostPlan &hp = pl->hp;
    int rc = JTP_OK;
    std::vector<JtTask> tasks;
    std::vector<JtBlock> blocks, ublocks;              // passes over belief tables; passes of cliques that keep none
    std::vector<int32_t> itab;
    std::vector<JtMargDesc> descs((size_t)n);
    std::vector<int64_t> elems((size_t)n);
    int64_t scratch_doubles = 0, total_out = 0;
    int lds = 0, ulds = 0;
    // Requests on ONE clique share passes over its belief table, JT_MAX_OUT of them per pass (a pairwise model asks a
    // clique for two or three factor marginals: round 3 read the table once per request - config 3: 1831 reads of 878
    // tables, 2.1 x the bytes).  Multi-set plans marginalise psi x messages directly and keep one request per task.
    std::vector<char> lean_later;                        // per task: a unit clique's marginals (single-set plans)
    for (int i = 0; i < n; ++i) {
        const int clique = cliques[i];
        if (clique < 0 || clique >= hp.n_cliques) return set_err(JTP_EINVAL, "request %d: node %d is not a clique", i, clique);
        if (!(hp.pn[clique].owner == hp.rank || hp.pn[clique].owner == hp.n_ranks)) return set_err(JTP_EINVAL, "clique %d belongs to rank %d", clique, hp.pn[clique].owner);
    }
    // (multi-set plans: one request per pass; unit cliques of single-set plans share passes like everybody else)
    const std::vector<std::vector<int>> groups = jtp_group_requests(cliques, n, hp.knobs.marg_group, pl->multiset);
    for (const std::vector<int> &grp : groups) {
        const int clique = cliques[grp[0]];
        std::vector<std::vector<int>> ovs;
        for (int i : grp) {
            const int n_out = var_off[i + 1] - var_off[i];
            if (n_out < 0 || n_out > JT_MAX_VARS) return set_err(JTP_EINVAL, "request %d: bad variable count", i);
            std::vector<int> ov(var_ids + var_off[i], var_ids + var_off[i + 1]);
            for (int a = 0; a < n_out; ++a) {
                if (ov[a] < 0 || ov[a] >= hp.n_vars) return set_err(JTP_EINVAL, "request %d: variable %d out of range", i, ov[a]);
                for (int c = 0; c < a; ++c)
                    if (ov[a] == ov[c]) return set_err(JTP_EINVAL, "request %d: variable %d requested twice", i, ov[a]);
            }
            ovs.push_back(ov);
        }
        JtTask tk;
        std::vector<int> out_bits, npart;
        std::vector<JtBlock> blk;
        std::vector<int32_t> tab;
        std::string err;
        const bool direct = pl->multiset || hp.pn[clique].unit;     // psi x incoming tables marginalised directly
        rc = jtp_plan_marginal_task(hp, clique, ovs, tk, tab, out_bits, npart, blk, err, direct);
        if (rc) return set_err(rc, "request %d: %s", grp[0], err.c_str());
        tk.itab_off = (int64_t)itab.size();
        if (tk.tmap_off >= 0) tk.tmap_off += tk.itab_off;      // (the clique's thread map travels behind the task's rows)
        itab.insert(itab.end(), tab.begin(), tab.end());
        for (JtBlock &bk : blk) {
            bk.task = (uint32_t)tasks.size();
            (direct ? ublocks : blocks).push_back(bk);
        }
        lean_later.push_back(direct && hp.pn[clique].unit && !pl->multiset);
        if (direct) ulds = std::max(ulds, tk.lds_bytes);
        else lds = std::max(lds, tk.lds_bytes);
        for (size_t j = 0; j < grp.size(); ++j) {
            const int i = grp[j];
            const std::vector<int> &ov = ovs[j];
            const int n_out = (int)ov.size();
            tk.msg[JT_MAX_IN + j].off = scratch_doubles;
            JtMargDesc md;
            memset(&md, 0, sizeof md);
            int bit = 0;
            std::vector<int> pos(n_out), nb(n_out);
            for (int a = n_out - 1; a >= 0; --a) {          // last requested variable = lowest bits
                pos[a] = bit;
                nb[a] = hp.vbits[ov[a]];
                bit += nb[a];
            }
            md.d = bitfield_desc(hp, ov, pos.data(), nb.data(), out_bits[j]);
            const int64_t stride = md.d.host_elems;
            md.src_off = scratch_doubles;
            md.pstride = (int64_t)1 << out_bits[j];
            md.npart = npart[j];
            descs[i] = md;
            elems[i] = stride;
            scratch_doubles += md.pstride * npart[j];
        }
        tasks.push_back(tk);
    }
    for (int i = 0; i < n; ++i) {                          // results in request order
        descs[i].dst_off = total_out;
        total_out += elems[i];
    }
    // (round 6) marginals of unit cliques run the lean pass: the records are made once every output's place is known
    for (size_t t = 0; t < tasks.size(); ++t)
        if (lean_later[t]) jtp_make_lean(hp, tasks[t], itab, true);
    // (their workgroups first in the list of the cliques that keep no table: a launch of jt_lean_single, then jt_single for the rest)
    std::stable_partition(ublocks.begin(), ublocks.end(), [&](const JtBlock &bk) { return tasks[bk.task].lean_off > 0; });
    int n_lean_blocks = 0, lean_lds = 0;
    for (const JtBlock &bk : ublocks)
        if (tasks[bk.task].lean_off > 0) ++n_lean_blocks, lean_lds = std::max(lean_lds, tasks[bk.task].lds_bytes);
    // (the tables of the list are complete before the plan sees them: a failure below leaves the cache as it was)
    made.reset(new MargBatch(&pl->mem));
    MargBatch *mb = made.get();
    mb->lean_nblocks = n_lean_blocks;
    mb->lean_lds = lean_lds;
    if (pl->multiset && pl->set0) mb->h_tasks = tasks;
    mb->key = key;
    mb->n = n;
    mb->nblocks = (int)blocks.size();
    mb->lds = lds;
    mb->unit_nblocks = (int)ublocks.size();
    mb->unit_lds = ulds;
    blocks.insert(blocks.end(), ublocks.begin(), ublocks.end());
    mb->total_out = total_out;
    mb->elems = elems;
    int64_t biggest = 1;
    for (int64_t e : elems) biggest = std::max(biggest, e);
    mb->max_grid_x = (int)std::min<int64_t>((biggest + 255) / 256, 64);
    HIP_TRY(mb->d_tasks.upload(tasks));
    HIP_TRY(mb->d_blocks.upload(blocks));
    HIP_TRY(mb->d_itab.upload(itab, 1));
    HIP_TRY(mb->d_descs.upload(descs));
    HIP_TRY(mb->scratch.alloc((size_t)std::max<int64_t>(scratch_doubles, 1)));
    HIP_TRY(mb->stage.alloc((size_t)std::max<int64_t>(total_out, 1)));
    // the plan's own list: where the folded tasks of the propagate leave these marginals
    if (!hp.folded.empty() && key == hp.fold_key && !pl->multiset) {
        bool all = true;
        std::vector<JtMargDesc> fd = descs;
        for (int i = 0; i < n; ++i) {
            const bool direct = hp.pn[cliques[i]].unit;
            const HostPlan::FoldReq &fr = hp.folded[i];
            if (!direct) continue;                             // (a belief table: jt_marginals, as ever)
            if (fr.task < 0 || fr.out_bits != fd[i].d.nbits) {
                all = false;
                break;
            }
            fd[i].src_off = fr.off;
            fd[i].pstride = (int64_t)1 << fr.out_bits;
            fd[i].npart = fr.npart;
            fd[i].in_arena = 1;
        }
        if (all) {
            HIP_TRY(mb->d_descs_fold.upload(fd));
            mb->folded = true;
        }
    }
    return JTP_OK;
}

// Formation launches of one evidence set for a request list (what jtp_get_marginals enqueues before its unpack, without the
// folded-marginal shortcut): the partial copies of every request into `scratch`, on the set's stream, from records `tasks`.
static int launch_formation(jtp_plan *pl, MargBatch *mb, int batch, const JtTask *tasks, double *scratch) {
    BatchBuffers &b = pl->bufs[batch];
    hipStream_t s = pl->streams[batch % pl->streams.size()];
    JtFlow plain = readout_flow();
    int rc = JTP_OK;
    if (mb->nblocks > 0) {
        rc = launch_readout(pl, JT_K_MARGINALS, mb->nblocks, mb->lds, s, tasks, mb->d_blocks.get(), mb->d_itab.get(), b.bel, b.bel, scratch, plain);
        if (rc) return rc;
    }
    if (mb->unit_nblocks > 0) {
        readout_inputs(plain, pl, b);
        plain.out_shift = (int64_t)(((intptr_t)scratch - (intptr_t)(b.msg + plain.cur_off)) / 8);
        const int n_lean = plain.ev == nullptr ? mb->lean_nblocks : 0;
        if (n_lean > 0) {
            rc = launch_readout(pl, JT_K_LEAN_SINGLE, n_lean, mb->lean_lds, s, tasks, mb->d_blocks.get() + mb->nblocks, mb->d_itab.get(), b.psi, b.bel, b.msg, plain);
            if (rc) return rc;
        }
        if (mb->unit_nblocks > n_lean) {
            rc = launch_readout(pl, JT_K_SINGLE, mb->unit_nblocks - n_lean, mb->unit_lds, s, tasks, mb->d_blocks.get() + mb->nblocks + n_lean, mb->d_itab.get(), b.psi, b.bel, b.msg, plain);
            if (rc) return rc;
        }
    }
    HIP_TRY(hipGetLastError());
    return JTP_OK;
}

// sum of the root belief as the device holds it (a JTP_SCALED plan: Z x 2^-E_root)
static int root_sum(jtp_plan *pl, int32_t batch, double *z) {
    if (!pl) return set_err(JTP_EINVAL, "null plan");
    if (!z) return set_err(JTP_EINVAL, "null argument");
    if (pl->hp.pn[pl->hp.root].owner != pl->hp.rank && pl->hp.pn[pl->hp.root].owner != pl->hp.n_ranks)
        return set_err(JTP_EINVAL, "the root clique belongs to rank %d", pl->hp.pn[pl->hp.root].owner);
    return jtp_get_marginal(pl, batch, pl->hp.root, nullptr, 0, z);
}

// JTP_SCALED plans: the exponents of the last propagate of evidence set `batch`, and from them the exponent of every node - a walk
// down the planner's own tree (re-rooted, virtual cliques included).  With U(c) = the sum of e_up over the subtree of c, the upward
// message of c is the true one x 2^-U(c); the root multiplies all of them: E_root = sum of every e_up.  The downward message into c
// carries what its parent's belief carries without c's own subtree, and its own exponent:
//     E_child = E_parent - e_up(child) + e_dn(child);      separator (up x down) = E_parent + e_dn(child) = E_child + e_up(child).
static size_t scale_words(const HostPlan &hp) { return std::max<size_t>(2 * hp.ps.size(), 1); }      // int32 per evidence set (BatchBuffers::exps)

// ... from the exponents of the set's last propagate, already on the host (`ex`: scale_words of them)
static void scale_from_exps(jtp_plan *pl, int batch, const int32_t *ex) {
    HostPlan &hp = pl->hp;
    BatchBuffers &b = pl->bufs[batch];
    const int np = (int)hp.pn.size();
    b.node_e.assign(np, 0);
    b.sep_e.assign(hp.ps.size(), 0);
    std::vector<int> order(np);
    for (int c = 0; c < np; ++c) order[c] = c;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return hp.pn[x].depth < hp.pn[y].depth; });
    int64_t all_up = 0;
    for (int c = 0; c < np; ++c)
        if (hp.pn[c].psep >= 0) all_up += ex[2 * hp.pn[c].psep];
    for (int c : order) {
        const PNode &p = hp.pn[c];
        if (p.psep < 0 || p.parent < 0) {
            b.node_e[c] = all_up;
            continue;
        }
        b.sep_e[p.psep] = b.node_e[p.parent] + ex[2 * p.psep + 1];
        b.node_e[c] = b.sep_e[p.psep] - ex[2 * p.psep];
    }
    b.scale_fresh = true;
}

static int fetch_scale(jtp_plan *pl, int batch) {
    HostPlan &hp = pl->hp;
    BatchBuffers &b = pl->bufs[batch];
    if (!hp.scaled || b.scale_fresh) return JTP_OK;
    int rc = settle(pl, batch);
    if (rc) return rc;
    hipStream_t s = pl->streams[batch % pl->streams.size()];
    std::vector<int32_t> ex(scale_words(hp), 0);
    HIP_TRY(hipMemcpyAsync(ex.data(), b.exps, ex.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    scale_from_exps(pl, batch, ex.data());
    return JTP_OK;
}

// ------------------------------------------------------------------------------------------ data out

extern "C" {

int jtp_get_belief(jtp_plan *pl, int32_t batch, int32_t node, void *host, int32_t host_dtype) {
    int rc = check_ready(pl, batch);
    if (rc) return rc;
    HostPlan &hp = pl->hp;
    if (node < 0 || node >= hp.n_nodes) return set_err(JTP_EINVAL, "node %d out of range", node);
    if (host_dtype != JTP_F32 && host_dtype != JTP_F64) return set_err(JTP_EINVAL, "bad host dtype");
    HIP_TRY(hipSetDevice(hp.device));
    roctx::Range range(pl->roctx, "jtp_get_belief");
    rc = settle(pl, batch);
    if (rc) return rc;
    hipStream_t s = pl->streams[batch % pl->streams.size()];
    BatchBuffers &b = pl->bufs[batch];
    const size_t hsz = host_dtype == JTP_F32 ? 4 : 8;
    if (node < hp.n_cliques) {
        if (!(hp.pn[node].owner == hp.rank || hp.pn[node].owner == hp.n_ranks)) return set_err(JTP_EINVAL, "clique %d belongs to rank %d", node, hp.pn[node].owner);
        const JtPackDesc &d = hp.pack[node];
        const bool unit = hp.pn[node].unit;
        const bool direct = pl->multiset || unit;
        // What the first call needs is built into locals and moved into the plan once ALL of it is there: a call that fails leaves
        // the plan as it found it.
        //  - a unit clique keeps no belief table either: formed now, into a scratch arena laid out as its table would be;
        //  - multi-set plans and unit cliques keep no belief tables: this clique's belief for this evidence set is formed now, from
        //    the shared table and the set's final messages (computation.py:216-224), by a task of its own.
        DeviceBuf<char> scratch(&pl->mem);
        jtp_plan::BeliefTask fresh(&pl->mem);
        if (unit && !pl->unit_scratch) HIP_TRY(scratch.alloc((size_t)hp.scratch_elems * pl->esize));
        if (direct && pl->belief_tasks.size() < hp.pn.size()) pl->belief_tasks.resize(hp.pn.size());
        if (direct && !pl->belief_tasks[node].d_task) {
            JtTask tk;
            std::vector<int32_t> itab;
            std::vector<JtBlock> blocks;
            std::string err;
            rc = jtp_plan_belief_task(hp, node, tk, itab, blocks, err);
            if (rc) return set_err(rc, "%s", err.c_str());
            HIP_TRY(fresh.d_task.upload(&tk, 1));
            HIP_TRY(fresh.d_blk.upload(blocks));
            HIP_TRY(fresh.d_tab.upload(itab, 1));
            fresh.h_task = tk;
            fresh.nblocks = (int)blocks.size();
            fresh.lds = tk.lds_bytes;
        }
        rc = ensure_stage(pl, (size_t)d.host_elems * hsz);
        if (rc) return rc;
        if (scratch) {
            pl->unit_scratch = std::move(scratch);
            HIP_TRY(hipMemsetAsync(pl->unit_scratch.get(), 0, pl->unit_scratch.bytes(), s));
        }
        if (fresh.d_task) pl->belief_tasks[node] = std::move(fresh);
        void *bel_src = unit ? (void *)pl->unit_scratch.get() : b.bel;
        if (direct) {
            jtp_plan::BeliefTask &bt = pl->belief_tasks[node];
            if (pl->multiset && pl->set0) {              // (which inputs come from the evidence-free set's arena depends on the set)
                JtTask patched = bt.h_task;
                readout_redirect(pl, batch, patched);
                HIP_TRY(hipStreamSynchronize(s));        // (an earlier read-out's kernel may still read the record)
                HIP_TRY(hipMemcpy(bt.d_task.get(), &patched, sizeof patched, hipMemcpyHostToDevice));
            }
            JtFlow one = readout_flow();
            readout_inputs(one, pl, b);
            rc = launch_readout(pl, JT_K_SINGLE, bt.nblocks, bt.lds, s, bt.d_task.get(), bt.d_blk.get(), bt.d_tab.get(), b.psi, bel_src, b.msg, one);
            if (rc) return rc;
            HIP_TRY(hipGetLastError());
        }
        const int grid = grid_1d(d.host_elems);
        if (hp.dtype == JTP_F32) {
            if (host_dtype == JTP_F32) hipLaunchKernelGGL((jt_unpack<float, float>), dim3(grid), dim3(256), 0, s, d, (const float *)bel_src, (float *)pl->stage.get());
            else hipLaunchKernelGGL((jt_unpack<float, double>), dim3(grid), dim3(256), 0, s, d, (const float *)bel_src, (double *)pl->stage.get());
        } else {
            if (host_dtype == JTP_F32) hipLaunchKernelGGL((jt_unpack<double, float>), dim3(grid), dim3(256), 0, s, d, (const double *)bel_src, (float *)pl->stage.get());
            else hipLaunchKernelGGL((jt_unpack<double, double>), dim3(grid), dim3(256), 0, s, d, (const double *)bel_src, (double *)pl->stage.get());
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host, pl->stage.get(), (size_t)d.host_elems * hsz, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return check_flow(pl, batch);
    }
    const int si = hp.sep_of_node[node];
    if (si < 0) return set_err(JTP_EINVAL, "separator node %d is not part of the tree", node);
    const PSep &sp = hp.ps[si];
    if (sp.up_off < 0) return set_err(JTP_EINVAL, "separator node %d is not held by rank %d", node, hp.rank);
    std::vector<int> pos, nb;                               // the separator's layout in the node's host axis order
    for (int v : hp.node_vars[node]) {
        int j = 0;
        while (sp.vars[j] != v) ++j;
        pos.push_back(sp.pos[j]);
        nb.push_back(sp.nb[j]);
    }
    const JtPackDesc d = bitfield_desc(hp, hp.node_vars[node], pos.data(), nb.data(), sp.nbits);
    const int64_t stride = d.host_elems;
    rc = ensure_stage(pl, (size_t)stride * hsz);
    if (rc) return rc;
    const int grid = grid_1d(stride);
    const int64_t pstride = (int64_t)1 << sp.nbits;
    const double *cur = b.msg + cur_half(pl, b);            // the half the last propagate wrote
    const double *cur_up = cur;
    if (pl->multiset && pl->set0 && !pl->member_host.empty() && sp.child >= 0 && hp.pn[sp.child].collect_task >= 0 &&
        !pl->member_host[(size_t)hp.pn[sp.child].collect_task * ((size_t)pl->n_groups * JT_MSETS) + (size_t)(pl->set0 + batch)])
        cur_up = pl->msg_all.get() + cur_half(pl, b);       // (readout_redirect: the evidence-free set's upward message)
    if (host_dtype == JTP_F32)
        hipLaunchKernelGGL((jt_msg_unpack<float>), dim3(grid), dim3(256), 0, s, d, cur_up + sp.up_roff, sp.up_rnpart, cur + sp.dn_roff, sp.dn_rnpart, pstride, (float *)pl->stage.get());
    else
        hipLaunchKernelGGL((jt_msg_unpack<double>), dim3(grid), dim3(256), 0, s, d, cur_up + sp.up_roff, sp.up_rnpart, cur + sp.dn_roff, sp.dn_rnpart, pstride, (double *)pl->stage.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host, pl->stage.get(), (size_t)stride * hsz, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return check_flow(pl, batch);
}

// One marginal = a request list of one (its device tables are kept with the plan like any other list's:
// no allocation per call, nothing to leak on an error path).
int jtp_get_marginal(jtp_plan *pl, int32_t batch, int32_t clique, const int32_t *out_vars, int32_t n_out, double *host) {
    int rc = check_ready(pl, batch);
    if (rc) return rc;
    if (n_out < 0 || n_out > JT_MAX_VARS || (n_out > 0 && !out_vars) || !host) return set_err(JTP_EINVAL, "bad variable list");
    if (clique < 0 || clique >= pl->hp.n_cliques) return set_err(JTP_EINVAL, "node %d is not a clique", clique);
    int64_t elems = 1;
    for (int i = 0; i < n_out; ++i) {
        if (out_vars[i] < 0 || out_vars[i] >= pl->hp.n_vars) return set_err(JTP_EINVAL, "variable %d out of range", out_vars[i]);
        elems *= pl->hp.card[out_vars[i]];
    }
    const int32_t var_off[2] = {0, n_out};
    const int64_t out_off[2] = {0, elems};
    const int32_t none = 0;
    return jtp_get_marginals(pl, batch, 1, &clique, var_off, n_out > 0 ? out_vars : &none, out_off, host);
}

int jtp_get_marginals(jtp_plan *pl, int32_t batch, int32_t n, const int32_t *cliques, const int32_t *var_off,
                      const int32_t *var_ids, const int64_t *out_off, double *host) {
    int rc = check_ready(pl, batch);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!cliques || !var_off || !out_off || !host))) return set_err(JTP_EINVAL, "null argument");
    if (n == 0) return JTP_OK;
    if (n > 65535) {                                        // grid.y of the read-out launch
        for (int32_t i = 0; i < n; i += 65535) {
            rc = jtp_get_marginals(pl, batch, std::min(65535, n - i), cliques + i, var_off + i, var_ids, out_off + i, host);
            if (rc) return rc;
        }
        return JTP_OK;
    }
    HostPlan &hp = pl->hp;
    HIP_TRY(hipSetDevice(hp.device));
    roctx::Range range(pl->roctx, "jtp_get_marginals");
    rc = settle(pl, batch);
    if (rc) return rc;
    hipStream_t s = pl->streams[batch % pl->streams.size()];
    BatchBuffers &b = pl->bufs[batch];
    const std::vector<int32_t> key = marg_key(n, cliques, var_off, var_ids);
    MargBatch *mb = find_marg_batch(pl, key);
    if (!mb) {
        std::unique_ptr<MargBatch> made;
        rc = make_marg_batch(pl, key, n, cliques, var_off, var_ids, made);
        if (rc) return rc;
        mb = keep_marg_batch(pl, made);
    }
    if (!mb->h_tasks.empty()) {                          // (multi-set plans with active lists: readout_redirect, per evidence set)
        std::vector<JtTask> patched = mb->h_tasks;
        for (JtTask &tk : patched) readout_redirect(pl, batch, tk);
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(mb->d_tasks.get(), patched.data(), patched.size() * sizeof(JtTask), hipMemcpyHostToDevice));
    }
    JtFlow plain = readout_flow();
    // marginalise the BELIEF tables: each is the "potential" argument of a childless collect
    if (mb->nblocks > 0) {
        rc = launch_readout(pl, JT_K_MARGINALS, mb->nblocks, mb->lds, s, mb->d_tasks.get(), mb->d_blocks.get(), mb->d_itab.get(), b.bel, b.bel, mb->scratch.get(), plain);
        if (rc) return rc;
    }
    // Marginals the propagate formed itself (fold_marginals): valid when the last propagate of this evidence set ran them - a dataflow
    // launch whose distribute segment is jt_propagate_flow, or one launch per level - and the set observes nothing (a clique that hosts
    // an observed variable has no lean pass).  Then only the belief-table requests are computed here.
    bool use_fold = false;
    if (mb->folded && !b.ev_any && b.epoch > 0) {
        if (pl->launch_mode == 0) use_fold = true;
        else {
            use_fold = !hp.segments.empty();
            for (const Segment &sg : hp.segments)
                if (sg.phase == 1 && (pl->chain || hp.tmix || !flow_both())) use_fold = false;
        }
    }
    if (mb->unit_nblocks > 0 && !use_fold) {
        // cliques that keep no belief table (multi-set plans: all; else the unit cliques): psi * (the incoming tables)
        // marginalised directly - inputs from the set's message arena (and the fixed arena), outputs into the request list's
        // scratch buffer (JtFlow::out_shift)
        readout_inputs(plain, pl, b);
        plain.out_shift = (int64_t)(((intptr_t)mb->scratch.get() - (intptr_t)(b.msg + plain.cur_off)) / 8);
        // (round 6) the tasks with a lean record through jt_lean_single while the evidence set observes nothing
        const int n_lean = plain.ev == nullptr ? mb->lean_nblocks : 0;
        if (n_lean > 0) {
            rc = launch_readout(pl, JT_K_LEAN_SINGLE, n_lean, mb->lean_lds, s, mb->d_tasks.get(), mb->d_blocks.get() + mb->nblocks, mb->d_itab.get(), b.psi, b.bel, b.msg, plain);
            if (rc) return rc;
        }
        if (mb->unit_nblocks > n_lean) {
            rc = launch_readout(pl, JT_K_SINGLE, mb->unit_nblocks - n_lean, mb->unit_lds, s, mb->d_tasks.get(), mb->d_blocks.get() + mb->nblocks + n_lean, mb->d_itab.get(), b.psi, b.bel, b.msg, plain);
            if (rc) return rc;
        }
    }
    hipLaunchKernelGGL(jt_marg_unpack, dim3(mb->max_grid_x, mb->n), dim3(256), 0, s, use_fold ? mb->d_descs_fold.get() : mb->d_descs.get(), mb->scratch.get(), mb->stage.get(),
                       (const double *)(b.msg + cur_half(pl, b)));
    HIP_TRY(hipGetLastError());
    bool packed = true;
    for (int i = 0; i < n; ++i) packed = packed && out_off[i + 1] - out_off[i] == mb->elems[i];
    if (packed) {
        HIP_TRY(hipMemcpyAsync(host + out_off[0], mb->stage.get(), (size_t)mb->total_out * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    } else {
        std::vector<double> tmp((size_t)mb->total_out);
        HIP_TRY(hipMemcpyAsync(tmp.data(), mb->stage.get(), (size_t)mb->total_out * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        int64_t at = 0;
        for (int i = 0; i < n; ++i) {
            memcpy(host + out_off[i], tmp.data() + at, (size_t)mb->elems[i] * 8);
            at += mb->elems[i];
        }
    }
    return check_flow(pl, batch);
}

int jtp_get_log2_scale(jtp_plan *pl, int32_t batch, int32_t node, int64_t *e) {
    if (!pl || !e) return set_err(JTP_EINVAL, "null argument");
    HostPlan &hp = pl->hp;
    if (node < 0 || node >= hp.n_nodes) return set_err(JTP_EINVAL, "node %d out of range", node);
    *e = 0;
    if (!hp.scaled) return JTP_OK;
    int rc = check_ready(pl, batch);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(hp.device));
    rc = fetch_scale(pl, batch);
    if (rc) return rc;
    if (node < hp.n_cliques) *e = pl->bufs[batch].node_e[node];
    else {
        const int si = hp.sep_of_node[node];
        if (si < 0) return set_err(JTP_EINVAL, "separator node %d is not part of the tree", node);
        *e = pl->bufs[batch].sep_e[si];
    }
    return JTP_OK;
}

int jtp_get_z(jtp_plan *pl, int32_t batch, double *z) {
    int rc = root_sum(pl, batch, z);
    if (rc || !pl->hp.scaled) return rc;
    rc = fetch_scale(pl, batch);
    if (rc) return rc;
    const int64_t e = pl->bufs[batch].node_e[pl->hp.root];
    *z = ldexp(*z, (int)std::min<int64_t>(std::max<int64_t>(e, -100000), 100000));       // (inf or 0 where Z is outside float64)
    return JTP_OK;
}

int jtp_get_log_z(jtp_plan *pl, int32_t batch, double *log_abs_z, int32_t *sign) {
    if (!log_abs_z || !sign) return set_err(JTP_EINVAL, "null argument");
    double sum = 0;
    int rc = root_sum(pl, batch, &sum);
    if (rc) return rc;
    int64_t e = 0;
    if (pl->hp.scaled) {
        rc = fetch_scale(pl, batch);
        if (rc) return rc;
        e = pl->bufs[batch].node_e[pl->hp.root];
    }
    *sign = (sum > 0) - (sum < 0);                      // (a NaN sum: sign 0, log NaN)
    *log_abs_z = log(fabs(sum)) + (e ? (double)e * 0.69314718055994530942 : 0.0);
    return JTP_OK;
}

// ------------------------------------------------------------------------------------------ expected counts

int jtp_accumulate_marginals(jtp_plan *pl, int32_t batch_begin, int32_t batch_end, const double *weights, int32_t n,
                             const int32_t *cliques, const int32_t *var_off, const int32_t *var_ids, const int64_t *out_off,
                             double *host, double *log_abs_z, int32_t *z_sign) {
    if (!pl) return set_err(JTP_EINVAL, "null plan");
    HostPlan &hp = pl->hp;
    if (hp.n_ranks > 1) return set_err(JTP_EUNSUPPORTED, "jtp_accumulate_marginals: the plan is one of %d ranks; the sum over evidence sets is formed on one device", hp.n_ranks);
    int rc = check_ready(pl, 0);
    if (rc) return rc;
    if (batch_begin < 0 || batch_end > hp.n_batch || batch_begin >= batch_end)
        return set_err(JTP_EINVAL, "evidence sets [%d,%d): not a range within [0,%d)", batch_begin, batch_end, hp.n_batch);
    if (n < 0 || (n > 0 && (!cliques || !var_off || !out_off || !host))) return set_err(JTP_EINVAL, "null argument");
    if (n > 0 && var_off[n] > var_off[0] && !var_ids) return set_err(JTP_EINVAL, "null argument");
    if ((log_abs_z == nullptr) != (z_sign == nullptr)) return set_err(JTP_EINVAL, "log_abs_z and z_sign: both or neither");
    const int64_t range = (int64_t)batch_end - batch_begin;
    if (weights)
        for (int64_t k = 0; k < range; ++k)
            if (!std::isfinite(weights[k])) return set_err(JTP_EINVAL, "weight of evidence set %d is not finite", (int)(batch_begin + k));
    if (hp.pn[hp.root].owner != hp.rank && hp.pn[hp.root].owner != hp.n_ranks) return set_err(JTP_EINVAL, "the root clique belongs to rank %d", hp.pn[hp.root].owner);
    HIP_TRY(hipSetDevice(hp.device));
    roctx::Range roctx_range(pl->roctx, "jtp_accumulate_marginals");
    for (int b = batch_begin; b < batch_end; ++b) {
        rc = settle(pl, b);
        if (rc) return rc;
    }
    // the list as the caller gave it, and behind it the root's scalar: S of that request is the root sum log Z comes from
    const int na = n + 1;
    std::vector<int32_t> cl(cliques, cliques + n), vo((size_t)na + 1), vi;
    cl.push_back(hp.root);
    for (int i = 0; i <= n; ++i) vo[i] = n > 0 ? var_off[i] - var_off[0] : 0;
    vo[na] = vo[n];
    if (n > 0) vi.assign(var_ids + var_off[0], var_ids + var_off[n]);
    vi.push_back(0);
    const std::vector<int32_t> key = marg_key(na, cl.data(), vo.data(), vi.data());
    MargBatch *mb = find_marg_batch(pl, key);
    std::unique_ptr<MargBatch> made;
    if (!mb) {
        rc = make_marg_batch(pl, key, na, cl.data(), vo.data(), vi.data(), made);
        if (rc) return rc;
        mb = made.get();
    }
    for (int i = 0; i < n; ++i)
        if (out_off[i + 1] - out_off[i] < mb->elems[i]) return set_err(JTP_EINVAL, "request %d: %lld entries, room for %lld", i, (long long)mb->elems[i], (long long)(out_off[i + 1] - out_off[i]));
    const int64_t total = mb->total_out - 1;                       // (the caller's entries: the root's scalar is the last)
    const int64_t slot_doubles = (int64_t)mb->scratch.size();
    int64_t chunk = pl->acc_chunk > 0 ? pl->acc_chunk : std::max<int64_t>(1, ((int64_t)64 << 20) / (slot_doubles * 8));
    chunk = std::min<int64_t>(std::min<int64_t>(chunk, range), 65535);        // (grid.y of jt_marg_sums)
    const size_t n_tasks = mb->h_tasks.size();                     // (> 0: the records differ from set to set, readout_redirect)
    // What this call needs beyond what the list holds is built into locals and moved in once ALL of it is there.
    MargBatch::Acc fresh(&pl->mem);
    const bool grow = mb->acc.slots < chunk || mb->acc.range < range;
    if (grow) {
        const int64_t slots = std::max(chunk, mb->acc.slots), rng = std::max(range, mb->acc.range);
        HIP_TRY(fresh.scratch.alloc((size_t)(slots * slot_doubles)));
        if (n_tasks) HIP_TRY(fresh.tasks.alloc((size_t)slots * n_tasks));
        HIP_TRY(fresh.entries.alloc((size_t)(slots * mb->total_out)));
        HIP_TRY(fresh.sums.alloc((size_t)(slots * na)));
        HIP_TRY(fresh.weights.alloc((size_t)rng));
        HIP_TRY(fresh.out.alloc((size_t)(total + rng + 2)));
        fresh.slots = slots;
        fresh.range = rng;
    }
    const size_t n_streams = pl->streams.size();
    if (pl->acc_ev.size() < n_streams) {
        std::vector<hipEvent_t> evs;
        for (size_t i = 0; i < n_streams; ++i) {
            hipEvent_t e = nullptr;
            const hipError_t err = hipEventCreateWithFlags(&e, hipEventDisableTiming);
            if (err != hipSuccess) {
                for (auto x : evs) (void)hipEventDestroy(x);
                HIP_TRY(err);
            }
            evs.push_back(e);
        }
        pl->acc_ev.swap(evs);
    }
    if (grow) mb->acc = std::move(fresh);
    if (made) mb = keep_marg_batch(pl, made);
    MargBatch::Acc &A = mb->acc;
    double *const d_out = A.out.get(), *const d_roots = d_out + total;
    unsigned long long *const d_bad = reinterpret_cast<unsigned long long *>(d_roots + range);
    hipStream_t sa = pl->streams[batch_begin % n_streams];         // the stream the sums and the accumulation run on
    // (nothing of an earlier call is in flight: every call ends with its streams waited for - below, `drain` on a failure)
    auto drain = [&]() { for (auto s : pl->streams) (void)hipStreamSynchronize(s); };
    if (weights) HIP_TRY(hipMemcpy(A.weights.get(), weights, (size_t)range * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)(total + range + 1) * 8, sa));
    HIP_TRY(hipMemsetAsync(d_bad + 1, 0xff, sizeof(unsigned long long), sa));
    std::vector<double> back((size_t)(total + range + 2));
    // (a scaled plan's logarithms need the exponents of every set's last propagate: copied behind the last chunk, when `sa` has
    //  waited for every stream of the range, and so for every propagate)
    const size_t n_ex = hp.scaled && log_abs_z ? scale_words(hp) : 0;
    std::vector<int32_t> exs(n_ex * (size_t)range);
    std::vector<char> ex_here(n_ex ? (size_t)range : 0, 0);
    std::vector<JtTask> patched;
    for (int64_t c0 = 0; c0 < range; c0 += chunk) {
        const int64_t cnt = std::min(chunk, range - c0);
        if (n_tasks) {                                            // every slot's records, uploaded once
            patched.resize((size_t)cnt * n_tasks);
            for (int64_t k = 0; k < cnt; ++k)
                for (size_t t = 0; t < n_tasks; ++t) {
                    JtTask &tk = patched[(size_t)k * n_tasks + t];
                    tk = mb->h_tasks[t];
                    readout_redirect(pl, (int)(batch_begin + c0 + k), tk);
                }
            HIP_TRY(hipMemcpy(A.tasks.get(), patched.data(), patched.size() * sizeof(JtTask), hipMemcpyHostToDevice));
        }
        std::vector<char> used(n_streams, 0);
        for (int64_t k = 0; k < cnt; ++k) {
            const int b = (int)(batch_begin + c0 + k);
            rc = launch_formation(pl, mb, b, n_tasks ? A.tasks.get() + (size_t)k * n_tasks : mb->d_tasks.get(), A.scratch.get() + k * slot_doubles);
            if (rc) {
                drain();
                return rc;
            }
            used[(size_t)b % n_streams] = 1;
        }
        hipError_t err = hipSuccess;
        for (size_t i = 0; i < n_streams && err == hipSuccess; ++i) {
            if (!used[i] || pl->streams[i] == sa) continue;
            err = hipEventRecord(pl->acc_ev[i], pl->streams[i]);
            if (err == hipSuccess) err = hipStreamWaitEvent(sa, pl->acc_ev[i], 0);
        }
        if (err == hipSuccess) {
            hipLaunchKernelGGL(jt_marg_sums, dim3((unsigned)na, (unsigned)cnt), dim3(256), 0, sa, mb->d_descs.get(), A.scratch.get(), slot_doubles, na,
                               A.entries.get(), mb->total_out, A.sums.get(), d_roots + c0);
            if (n > 0)
                hipLaunchKernelGGL(jt_marg_accumulate, dim3((unsigned)n, (unsigned)mb->max_grid_x), dim3(256), 0, sa, mb->d_descs.get(), A.entries.get(), mb->total_out, na,
                                   A.sums.get(), weights ? A.weights.get() + c0 : nullptr, (int)cnt, c0, d_out, d_bad);
            err = hipGetLastError();
        }
        if (c0 + cnt == range) {
            for (int64_t k = 0; k < range && n_ex && err == hipSuccess; ++k)
                if (!pl->bufs[batch_begin + k].scale_fresh) {
                    err = hipMemcpyAsync(exs.data() + (size_t)k * n_ex, pl->bufs[batch_begin + k].exps, n_ex * sizeof(int32_t), hipMemcpyDeviceToHost, sa);
                    ex_here[(size_t)k] = 1;
                }
            if (err == hipSuccess) err = hipMemcpyAsync(back.data(), d_out, back.size() * 8, hipMemcpyDeviceToHost, sa);
        }
        if (err == hipSuccess) err = hipStreamSynchronize(sa);   // (the one host wait of the chunk: its slots are the next chunk's)
        if (err != hipSuccess) {
            drain();
            HIP_TRY(err);
        }
    }
    for (size_t i = 0; i < n_streams && i < (size_t)range; ++i) {   // (every stream used has been waited for, through `sa`)
        rc = check_flow(pl, (int)(batch_begin + (int64_t)i));
        if (rc) return rc;
    }
    int64_t at = 0;
    for (int i = 0; i < n; ++i) {
        memcpy(host + out_off[i], back.data() + at, (size_t)mb->elems[i] * 8);
        at += mb->elems[i];
    }
    if (log_abs_z)
        for (int64_t k = 0; k < range; ++k) {
            const double sum = back[(size_t)(total + k)];
            int64_t e = 0;
            if (hp.scaled) {
                if (!pl->bufs[batch_begin + k].scale_fresh && ex_here[(size_t)k]) scale_from_exps(pl, (int)(batch_begin + k), exs.data() + (size_t)k * n_ex);
                rc = fetch_scale(pl, (int)(batch_begin + k));      // (nothing to do, unless check_flow had to run the set again)
                if (rc) return rc;
                e = pl->bufs[batch_begin + k].node_e[hp.root];
            }
            z_sign[k] = (sum > 0) - (sum < 0);
            log_abs_z[k] = log(fabs(sum)) + (e ? (double)e * 0.69314718055994530942 : 0.0);
        }
    unsigned long long bad[2];
    memcpy(bad, back.data() + total + range, sizeof bad);
    if (bad[0])
        return set_err(JTP_EINVAL, "jtp_accumulate_marginals: %llu (evidence set, request) pairs had a marginal without mass (a sum that is zero or not finite), "
                                   "the first: evidence set %d, request %d; they contribute nothing (evidence of probability zero? tables that overflowed "
                                   "on a plan without JTP_SCALED?)", bad[0], (int)(batch_begin + (int64_t)(bad[1] / (unsigned long long)na)), (int)(bad[1] % (unsigned long long)na));
    return JTP_OK;
}

}  // extern "C"
