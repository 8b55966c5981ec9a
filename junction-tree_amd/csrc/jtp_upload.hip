// Data in: clique potentials (packed from host arrays, evaluated from factor tables, synthetic), hard evidence, and the
// active lists of multi-set plans that follow the evidence.  Layout conversion is off the hot path.
#include <climits>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "jtp_engine.h"

// ------------------------------------------------------------------------------------------ kernels: layout conversion, synthetic fill

// digit of variable i at device (physical) element index x: a shift where the variable is a bit field
__device__ __forceinline__ int jt_digit(const JtPackDesc &d, int i, uint32_t x) {
    const uint32_t ds = d.dstride[i];
    if (d.row_elems > 0 && i == d.split_var)               // the variable across the thread part's top bit: low digit of the row, high digit above
        return (int)(((x % (uint32_t)d.row_elems) / ds) % (uint32_t)d.dmod[i]) + ((int)((x / d.split_ds2) % (uint32_t)d.split_mod2) << d.split_lb);
    if (d.row_elems > 0 && d.pos[i] < d.low_bits)          // a mixed-radix digit of the row (thread part at true cardinalities)
        return ds > 0 ? (int)(((x % (uint32_t)d.row_elems) / ds) % (uint32_t)d.dmod[i]) : 0;
    if (ds == (1u << d.pos[i]) && d.dmod[i] == (1 << d.nb[i])) return (int)((x >> d.pos[i]) & ((1u << d.nb[i]) - 1u));
    return ds > 0 ? (int)((x / ds) % (uint32_t)d.dmod[i]) : 0;
}

// device index -> host index; returns false for entries that name no table entry (padding inside the thread part)
__device__ __forceinline__ bool jt_dev_to_host(const JtPackDesc &d, uint32_t x, int64_t &hidx) {
    bool valid = true;
    int64_t h = 0, back = 0;
    for (int i = 0; i < d.nvars; ++i) {
        const int digit = jt_digit(d, i, x);
        valid = valid && (digit < d.card[i]);
        h += (int64_t)digit * d.hstride[i];
        if (d.row_elems > 0 && i == d.split_var)
            back += (int64_t)(digit & ((1 << d.split_lb) - 1)) * d.dstride[i] + (int64_t)(digit >> d.split_lb) * d.split_ds2;
        else
        back += (int64_t)digit * d.dstride[i];
    }
    if (back != (int64_t)x) valid = false;              // index bits no variable owns must be clear
    hidx = h;
    return valid;
}

// MODE 0: arena[x] = stage[host index] (pack);  MODE 1: synthetic fill
// MODE 2: 1 where the index names an entry, else 0 (tables of virtual cliques)
template <typename T, typename S, int MODE>
__global__ __launch_bounds__(256) void jt_pack(JtPackDesc d, const S *__restrict__ stage, T *__restrict__ arena,
                                               uint64_t key, double scale) {
    const int64_t n = d.phys_elems;
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += (int64_t)gridDim.x * blockDim.x) {
        int64_t h;
        const bool valid = jt_dev_to_host(d, (uint32_t)x, h);
        double v = 0.0;
        if (valid) {
            if constexpr (MODE == 0) v = (double)stage[h];
            else if constexpr (MODE == 2) v = 1.0;
            else {
                const uint64_t bits = jt_splitmix64(key + (uint64_t)h);
                v = (0.5 + (double)(bits >> 11) * (1.0 / 9007199254740992.0)) * scale;
            }
        }
        arena[d.dev_off + x] = (T)v;
    }
}

// Clique potentials = products of factor tables, written in the cliques' device layouts: CliqueGraph.evaluate
// (junctiontree/junctiontree.py:203-226) for a LIST of cliques in ONE launch (jtp_set_potential_products).
// Bound: HBM writes (sizeof(T) per element; the factor tables are small and sit in LDS, or are gathered through L2).
// A workgroup forms JT_EVAL_ROWS consecutive stored rows of one clique.  The element at x = row * row_len + t has
// digit_i(x) = digit_i(t) + digit_i(row * row_len) for every variable i (jt_digit is additive over the two parts: a variable
// lies inside the row, above it, or - one variable at most, JtEvalTask::straddle - has a low part inside and a high part
// above), so every factor's table index is tin[f](t) + rin[f](row): the divisions happen once per thread and once per
// row.  (Round 3's jt_eval_product decoded every element: 9.2 GiB of config-3 tables in 31 ms, 0.3 TB/s.)
template <typename T>
__global__ __launch_bounds__(256) void jt_eval_batch(const JtEvalTask *__restrict__ tasks, const int32_t *__restrict__ blk_start, int ntasks,
                                                     const JtEvalVar *__restrict__ fvars, const char *__restrict__ stage, T *__restrict__ arena) {
    constexpr int VEC = 16 / sizeof(T);
    typedef T ext_t __attribute__((ext_vector_type(VEC)));
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *lds_tab = reinterpret_cast<double *>(smem);
    __shared__ int32_t s_rin[JT_EVAL_ROWS][JT_EVAL_MAX_F];
    __shared__ int32_t s_rdig[JT_EVAL_ROWS], s_rok[JT_EVAL_ROWS];
    // (the records are read from memory, not passed as kernel arguments: hipcc (ROCm 7.2) mis-read the 32-bit arrays of a
    //  kernel-argument struct when indexed with a run-time index - dstride[cvar] came back as dstride[0])
    int lo = 0, hi = ntasks;
    const int b = (int)blockIdx.x;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk_start[mid] <= b) lo = mid;
        else hi = mid;
    }
    const JtEvalTask &tk = tasks[lo];
    const JtPackDesc &c = tk.clique;
    const int tid = (int)threadIdx.x;
    const int row0 = (b - blk_start[lo]) * JT_EVAL_ROWS;
    const int nrows = tk.n_rows - row0 < JT_EVAL_ROWS ? tk.n_rows - row0 : JT_EVAL_ROWS;
    const int L = tk.row_len, nf = tk.nf, sv = tk.straddle;
    const int scard = sv >= 0 ? c.card[sv] : 1;
    // small factor tables -> LDS, as doubles
#pragma unroll
    for (int f = 0; f < JT_EVAL_MAX_F; ++f) {
        if (f >= nf || tk.flds[f] < 0) continue;
        double *dst = lds_tab + tk.flds[f];
        const int n = tk.felems[f];
        if (tk.fis64[f]) {
            const double *src = reinterpret_cast<const double *>(stage) + tk.foff[f];
            for (int i = tid; i < n; i += 256) dst[i] = src[i];
        } else {
            const float *src = reinterpret_cast<const float *>(stage) + tk.foff[f];
            for (int i = tid; i < n; i += 256) dst[i] = (double)src[i];
        }
    }
    // place x (x = t inside the first row, or x = row * row_len) -> is it the part of a table entry, the straddling
    // variable's part of its digit, and every factor's part of its table index
    auto decode = [&](const uint32_t x, const bool high, int &sdig, int (&fidx)[JT_EVAL_MAX_F]) {
        bool ok = true;
        int64_t back = 0;
        sdig = 0;
        for (int i = 0; i < c.nvars; ++i) {
            const int d = jt_digit(c, i, x);
            if (i == sv) sdig = d;
            else ok = ok && d < c.card[i];
            if (c.row_elems > 0 && i == c.split_var)
                back += high ? (int64_t)(d >> c.split_lb) * c.split_ds2 : (int64_t)d * c.dstride[i];
            else
                back += (int64_t)d * c.dstride[i];
        }
        ok = ok && back == (int64_t)x;          // index bits no variable owns must be clear
#pragma unroll
        for (int f = 0; f < JT_EVAL_MAX_F; ++f) {
            int idx = 0;
            if (f < nf && ok) {
                const JtEvalVar *fv = fvars + tk.fv_off[f];
                for (int j = 0; j < tk.fnv[f]; ++j) {
                    const uint32_t ds = fv[j].ds;
                    const uint32_t xr = fv[j].kind ? x % (uint32_t)c.row_elems : x;
                    int digit = ds > 0 ? (int)((xr / ds) % (uint32_t)fv[j].mod) : 0;
                    if (fv[j].kind == 2) digit += (int)((x / c.split_ds2) % (uint32_t)c.split_mod2) << c.split_lb;
                    idx += digit * fv[j].stride;
                }
            }
            fidx[f] = idx;
        }
        return ok;
    };
    int tin[VEC][JT_EVAL_MAX_F], tdig[VEC];
    bool tok[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        const int t = tid * VEC + e;
        tok[e] = decode((uint32_t)(t < L ? t : 0), false, tdig[e], tin[e]) && t < L;
    }
    if (tid < nrows) {
        int hd, rin[JT_EVAL_MAX_F];
        const bool ok = decode((uint32_t)(row0 + tid) * (uint32_t)L, true, hd, rin);
        s_rok[tid] = ok ? 1 : 0;
        s_rdig[tid] = hd;
#pragma unroll
        for (int f = 0; f < JT_EVAL_MAX_F; ++f) s_rin[tid][f] = rin[f];
    }
    __syncthreads();
    const bool active = tid * VEC < L;
    T *row = arena + c.dev_off + (int64_t)row0 * L + tid * VEC;
    for (int r = 0; r < nrows; ++r, row += L) {
        const bool rok = s_rok[r] != 0;
        const int hd = s_rdig[r];
        bool ok[VEC];
        double v[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            ok[e] = tok[e] && rok && tdig[e] + hd < scard;
            v[e] = 1.0;
        }
        if (tk.accumulate && active) {
            const ext_t old = *reinterpret_cast<const ext_t *>(row);
#pragma unroll
            for (int e = 0; e < VEC; ++e) v[e] = (double)old[e];
        }
#pragma unroll
        for (int f = 0; f < JT_EVAL_MAX_F; ++f) {
            if (f >= nf) continue;
            const int ri = s_rin[r][f];
            if (tk.flds[f] >= 0) {
                const double *tab = lds_tab + tk.flds[f];
#pragma unroll
                for (int e = 0; e < VEC; ++e) v[e] *= tab[ok[e] ? tin[e][f] + ri : 0];
            } else if (tk.fis64[f]) {
                const double *tab = reinterpret_cast<const double *>(stage) + tk.foff[f];
#pragma unroll
                for (int e = 0; e < VEC; ++e) v[e] *= tab[ok[e] ? tin[e][f] + ri : 0];
            } else {
                const float *tab = reinterpret_cast<const float *>(stage) + tk.foff[f];
#pragma unroll
                for (int e = 0; e < VEC; ++e) v[e] *= (double)tab[ok[e] ? tin[e][f] + ri : 0];
            }
        }
        if (active) {
            ext_t ov;
#pragma unroll
            for (int e = 0; e < VEC; ++e) ov[e] = ok[e] ? (T)v[e] : (T)0;
            __builtin_nontemporal_store(ov, reinterpret_cast<ext_t *>(row));
        }
    }
}

// Evidence-free subtrees: the entries of the (task, slot) pairs that LEAVE an active list become "unwritten" again (JtFanout,
// rebuild_active).  (fl.oth_off: the distance of the second arena half from the first)
__global__ __launch_bounds__(256) void jt_multi_fanout(const JtFanout *__restrict__ list, double *__restrict__ msg, JtFlow fl) {
    const JtFanout f = list[blockIdx.x];
    if (!(f.flags & JT_FANOUT_RESET)) return;
    for (int i = threadIdx.x; i < f.count; i += 256)
#pragma unroll
        for (int s = 0; s < JT_MSETS; ++s) {
            if (f.slot[s] == 0xffffu) continue;
            double *base = msg + (int64_t)f.slot[s] * fl.set_stride + f.off + i;
            base[0] = __longlong_as_double((long long)JT_UNWRITTEN);
            base[fl.oth_off] = __longlong_as_double((long long)JT_UNWRITTEN);
        }
}

// ------------------------------------------------------------------------------------------ potentials

// potentials are written through evidence set 0 when the plan shares them
static int check_writable(jtp_plan *pl, int batch) {
    if ((pl->hp.flags & JTP_SHARE_POTENTIALS) && batch != 0)
        return set_err(JTP_EINVAL, "the plan shares its potentials between evidence sets: set them through evidence set 0");
    return JTP_OK;
}

template <typename T, typename S>
static void launch_pack(const JtPackDesc &d, const S *stage, T *arena, hipStream_t s) {
    hipLaunchKernelGGL((jt_pack<T, S, 0>), dim3(grid_1d(d.phys_elems)), dim3(256), 0, s, d, stage, arena, 0ull, 0.0);
}

// tables of virtual cliques: 1 where the index names an entry, else 0 (jtp_plan_create)
void launch_virtual_fill(const HostPlan &hp, const JtPackDesc &d, void *psi, hipStream_t s) {
    const int grid = grid_1d(d.phys_elems);
    if (hp.dtype == JTP_F32) hipLaunchKernelGGL((jt_pack<float, float, 2>), dim3(grid), dim3(256), 0, s, d, (const float *)nullptr, (float *)psi, 0ull, 1.0);
    else hipLaunchKernelGGL((jt_pack<double, double, 2>), dim3(grid), dim3(256), 0, s, d, (const double *)nullptr, (double *)psi, 0ull, 1.0);
}

static uint64_t host_splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

extern "C" {

int jtp_set_potential(jtp_plan *pl, int32_t batch, int32_t node, const void *host, const int64_t *shape,
                      int32_t host_dtype) {
    int rc = check_ready(pl, batch);
    if (rc) return rc;
    rc = check_writable(pl, batch);
    if (rc) return rc;
    pl->psi_dirty = true;
    HostPlan &hp = pl->hp;
    if (node < 0 || node >= hp.n_cliques) return set_err(JTP_EINVAL, "node %d is not a clique", node);
    if (!(hp.pn[node].owner == hp.rank || hp.pn[node].owner == hp.n_ranks)) return set_err(JTP_EINVAL, "clique %d belongs to rank %d", node, hp.pn[node].owner);
    if (host_dtype != JTP_F32 && host_dtype != JTP_F64) return set_err(JTP_EINVAL, "bad host dtype");
    // a unit clique (jtp_tree_desc.cover_*) keeps its potential as a static table over the covered variables: the other axes
    // of the host array must have length 1, as the reference's evaluate leaves them (junctiontree.py:52-61)
    const bool unit = hp.pn[node].unit;
    if (unit && hp.pn[node].stat < 0) {
        bool one = true;
        for (size_t i = 0; i < hp.node_vars[node].size(); ++i) one = one && (!shape || shape[i] == 1 || hp.card[hp.node_vars[node][i]] == 1);
        if (!shape) for (int v : hp.node_vars[node]) one = one && hp.card[v] == 1;
        const double v = !host ? 0.0 : (host_dtype == JTP_F32 ? (double)*(const float *)host : *(const double *)host);
        if (!one || v != 1.0)
            return set_err(JTP_EINVAL, "clique %d was described as depending on none of its variables (jtp_tree_desc.cover_*): its potential is 1", node);
        return JTP_OK;
    }
    JtPackDesc d = unit ? hp.stat_pack[node] : hp.pack[node];
    int64_t stride = 1;
    for (int i = d.nvars - 1; i >= 0; --i) {
        const int64_t len = shape ? shape[i] : d.card[i];
        if (len != d.card[i] && len != 1) {
            if (unit && len == hp.card[hp.node_vars[node][i]])
                return set_err(JTP_EINVAL, "clique %d axis %d has length %lld, but the clique was described as not depending on that variable (jtp_tree_desc.cover_*)", node, i, (long long)len);
            return set_err(JTP_EINVAL, "clique %d axis %d has length %lld, expected %d or 1", node, i, (long long)len, d.card[i]);
        }
        d.hstride[i] = (len == 1) ? 0 : stride;
        stride *= len;
    }
    const size_t hbytes = (size_t)stride * (host_dtype == JTP_F32 ? 4 : 8);
    HIP_TRY(hipSetDevice(hp.device));
    const int ui = (int)(pl->up_cursor++ & 1u);
    if (!pl->up_ev[ui]) HIP_TRY(hipEventCreateWithFlags(&pl->up_ev[ui], hipEventDisableTiming));
    if (pl->up_busy[ui]) {                                  // the pack kernel that read this buffer two calls ago
        HIP_TRY(hipEventSynchronize(pl->up_ev[ui]));
        pl->up_busy[ui] = false;
    }
    HIP_TRY(pl->up_stage[ui].reserve(std::max<size_t>(hbytes, 256)));
    void *stage = pl->up_stage[ui].get();
    hipStream_t s = pl->streams[batch % pl->streams.size()];
    // (from pageable memory the copy returns once the runtime has staged the caller's bytes; from page-locked
    //  memory - jtp_host_alloc - it is asynchronous and the caller must keep the array alive until jtp_sync)
    HIP_TRY(hipMemcpyAsync(stage, host, hbytes, hipMemcpyHostToDevice, s));
    BatchBuffers &b = pl->bufs[batch];
    if (unit) {
        if (host_dtype == JTP_F32) launch_pack<double, float>(d, (const float *)stage, b.fix, s);
        else launch_pack<double, double>(d, (const double *)stage, b.fix, s);
    } else if (hp.dtype == JTP_F32) {
        if (host_dtype == JTP_F32) launch_pack<float, float>(d, (const float *)stage, (float *)b.psi, s);
        else launch_pack<float, double>(d, (const double *)stage, (float *)b.psi, s);
    } else {
        if (host_dtype == JTP_F32) launch_pack<double, float>(d, (const float *)stage, (double *)b.psi, s);
        else launch_pack<double, double>(d, (const double *)stage, (double *)b.psi, s);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(pl->up_ev[ui], s));
    pl->up_busy[ui] = true;
    return JTP_OK;
}

// CliqueGraph.evaluate (junctiontree.py:203-226) for a list of cliques: ONE host-to-device copy of every factor table and
// of the kernel's records, ONE launch of jt_eval_batch over all the cliques (plus one per further JT_EVAL_MAX_F factors of
// the clique with the most).  Round 3 ran a copy and a launch per clique, and a kernel that decoded every element.
int jtp_set_potential_products(jtp_plan *pl, int32_t batch, int32_t n, const int32_t *cliques, const int32_t *factor_off,
                               const jtp_factor *factors) {
    int rc = check_ready(pl, batch);
    if (rc) return rc;
    rc = check_writable(pl, batch);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!cliques || !factor_off))) return set_err(JTP_EINVAL, "null argument");
    if (n == 0) return JTP_OK;
    HostPlan &hp = pl->hp;
    if (factor_off[0] < 0) return set_err(JTP_EINVAL, "bad factor list");
    const int32_t f0 = factor_off[0], nfact = factor_off[n] - f0;
    if (nfact < 0 || (nfact > 0 && !factors)) return set_err(JTP_EINVAL, "bad factor list");
    // the tables in the staging buffer: 8-byte slots so that f32 and f64 tables can mix
    std::vector<int64_t> offs((size_t)nfact), elems((size_t)nfact);
    size_t tbytes = 0;
    int npass = 1;
    std::vector<char> listed((size_t)hp.n_cliques, 0);
    for (int i = 0; i < n; ++i) {
        const int clique = cliques[i];
        if (clique < 0 || clique >= hp.n_cliques) return set_err(JTP_EINVAL, "node %d is not a clique", clique);
        // (every listed clique is formed by workgroups of ONE launch: a clique listed twice would be written by two of them)
        if (listed[clique]) return set_err(JTP_EINVAL, "clique %d is listed twice", clique);
        listed[clique] = 1;
        if (!(hp.pn[clique].owner == hp.rank || hp.pn[clique].owner == hp.n_ranks)) return set_err(JTP_EINVAL, "clique %d belongs to rank %d", clique, hp.pn[clique].owner);
        if (factor_off[i + 1] < factor_off[i]) return set_err(JTP_EINVAL, "bad factor list");
        const std::vector<int> &cvars = hp.node_vars[clique];
        npass = std::max(npass, (factor_off[i + 1] - factor_off[i] + JT_EVAL_MAX_F - 1) / JT_EVAL_MAX_F);
        for (int f = factor_off[i]; f < factor_off[i + 1]; ++f) {
            const jtp_factor &ft = factors[f];
            const int fi = f - factor_off[i];
            if (ft.n_vars < 0 || ft.n_vars > JT_MAX_VARS) return set_err(JTP_EINVAL, "factor %d: bad variable count", fi);
            if (ft.dtype != JTP_F32 && ft.dtype != JTP_F64) return set_err(JTP_EINVAL, "factor %d: bad dtype", fi);
            if (!ft.host || (ft.n_vars > 0 && !ft.var_ids)) return set_err(JTP_EINVAL, "factor %d: null argument", fi);
            int64_t ne = 1;
            for (int j = 0; j < ft.n_vars; ++j) {
                const int v = ft.var_ids[j];
                bool found = false;
                for (int cv : cvars) found = found || cv == v;
                if (!found) return set_err(JTP_EINVAL, "factor %d: variable %d is not in clique %d", fi, v, clique);
                const int64_t len = ft.shape ? ft.shape[j] : hp.card[v];
                if (len != hp.card[v] && len != 1) return set_err(JTP_EINVAL, "factor %d axis %d has length %lld, expected %d or 1", fi, j, (long long)len, hp.card[v]);
                if (hp.pn[clique].unit && len != 1) {
                    bool covered = false;
                    for (int cv : hp.pn[clique].cover) covered = covered || cv == v;
                    if (!covered) return set_err(JTP_EINVAL, "factor %d: clique %d was described as not depending on variable %d (jtp_tree_desc.cover_*)", fi, clique, v);
                }
                ne *= len;
            }
            if (hp.pn[clique].unit && hp.pn[clique].stat < 0)
                return set_err(JTP_EINVAL, "clique %d was described as depending on none of its variables (jtp_tree_desc.cover_*): it takes no factor", clique);
            elems[f - f0] = ne;
            offs[f - f0] = (int64_t)(tbytes / 8);
            tbytes += (size_t)((ne * (ft.dtype == JTP_F32 ? 4 : 8) + 7) / 8) * 8;
        }
    }
    pl->psi_dirty = true;
    HIP_TRY(hipSetDevice(hp.device));
    hipStream_t s = pl->streams[batch % pl->streams.size()];
    BatchBuffers &b = pl->bufs[batch];
    // the kernel's records: per pass the clique records, then the workgroup prefix sums
    // (lists [0, npass): cliques that keep a table, formed in the potential arena in its storage type; [npass, 2 npass): static
    //  tables of unit cliques, plain bit fields of doubles in the fixed arena)
    std::vector<std::vector<JtEvalTask>> tasks((size_t)npass * 2);
    std::vector<JtEvalVar> fvars;
    int lds_doubles = 0;
    for (int i = 0; i < n; ++i) {
        const int clique = cliques[i];
        const std::vector<int> &cvars = hp.node_vars[clique];
        const PNode &p = hp.pn[clique];
        const int nfc = factor_off[i + 1] - factor_off[i];
        int done = 0, pass = 0;
        if (p.unit && p.stat < 0) continue;                 // all ones, nothing stored
        do {
            JtEvalTask tk;
            memset(&tk, 0, sizeof tk);
            tk.clique = p.unit ? hp.stat_pack[clique] : hp.pack[clique];
            if (p.unit) tk.clique.low_bits = std::min(tk.clique.nbits, 9);      // (rows of at most 512 doubles: a 16-byte vector per thread)
            tk.accumulate = done > 0;
            tk.nf = std::min(nfc - done, JT_EVAL_MAX_F);
            tk.row_len = tk.clique.row_elems > 0 ? tk.clique.row_elems : 1 << tk.clique.low_bits;
            tk.n_rows = (int32_t)(tk.clique.phys_elems / tk.row_len);
            // the variable with a digit part inside the row and one above it
            tk.straddle = tk.clique.row_elems > 0 ? tk.clique.split_var : -1;
            if (tk.clique.row_elems == 0)
                for (int j = 0; j < tk.clique.nvars; ++j)
                    if (tk.clique.pos[j] < tk.clique.low_bits && tk.clique.pos[j] + tk.clique.nb[j] > tk.clique.low_bits) tk.straddle = j;
            int used = 0;
            for (int k = 0; k < tk.nf; ++k) {
                const int f = factor_off[i] + done + k;
                const jtp_factor &ft = factors[f];
                tk.fnv[k] = ft.n_vars;
                tk.fis64[k] = ft.dtype == JTP_F64;
                tk.foff[k] = ft.dtype == JTP_F64 ? offs[f - f0] : offs[f - f0] * 2;     // in elements of its own type
                tk.felems[k] = (int32_t)std::min<int64_t>(elems[f - f0], INT32_MAX);
                tk.flds[k] = -1;
                if (used + elems[f - f0] <= JT_EVAL_LDS_DOUBLES) {
                    tk.flds[k] = used;
                    used += (int)((elems[f - f0] + 1) & ~(int64_t)1);
                }
                tk.fv_off[k] = (int32_t)fvars.size();
                fvars.resize(fvars.size() + (size_t)ft.n_vars);
                JtEvalVar *fv = fvars.data() + tk.fv_off[k];
                int64_t stride = 1;
                for (int j = ft.n_vars - 1; j >= 0; --j) {
                    const int v = ft.var_ids[j];
                    int pos = 0;
                    while (cvars[pos] != v) ++pos;
                    const JtPackDesc &cd = tk.clique;
                    fv[j].ds = cd.dstride[pos];
                    fv[j].mod = cd.dmod[pos];
                    fv[j].kind = cd.row_elems > 0 && cd.pos[pos] < cd.low_bits ? (pos == cd.split_var ? 2 : 1) : 0;
                    const int64_t len = ft.shape ? ft.shape[j] : hp.card[v];
                    fv[j].stride = (len == 1) ? 0 : (int32_t)stride;
                    stride *= len;
                }
            }
            lds_doubles = std::max(lds_doubles, used);
            tasks[(p.unit ? npass : 0) + pass].push_back(tk);
            done += tk.nf;
            ++pass;
        } while (done < nfc);
        (void)p;
    }
    const int nlists = 2 * npass;
    std::vector<size_t> task_at((size_t)nlists), blk_at((size_t)nlists);
    size_t bytes = 0;
    for (int k = 0; k < nlists; ++k) {
        task_at[k] = bytes;
        bytes += (tasks[k].size() * sizeof(JtEvalTask) + 255) & ~(size_t)255;
        blk_at[k] = bytes;
        bytes += ((tasks[k].size() + 1) * sizeof(int32_t) + 255) & ~(size_t)255;
    }
    const size_t fvars_at = bytes;
    bytes += std::max<size_t>((fvars.size() * sizeof(JtEvalVar) + 255) & ~(size_t)255, 256);
    const size_t tables_at = bytes;
    bytes += std::max<size_t>((tbytes + 255) & ~(size_t)255, 256);
    if (pl->eval_pending && pl->eval_stream != s) {        // another evidence set's kernels may still read the buffer
        HIP_TRY(hipStreamSynchronize(pl->eval_stream));
        pl->eval_pending = false;
        pl->eval_cursor = 0;
    }
    if (pl->eval_cursor + bytes > pl->eval_stage.size()) {
        if (pl->eval_pending) HIP_TRY(hipStreamSynchronize(pl->eval_stream));
        pl->eval_pending = false;
        pl->eval_cursor = 0;
        if (bytes > pl->eval_stage.size()) {               // (the pair is there whole or not at all)
            const size_t want = std::max<size_t>(bytes, (size_t)8 << 20);
            pl->eval_host.reset();
            hipError_t e = pl->eval_stage.alloc(want);
            if (e == hipSuccess) e = pl->eval_host.alloc(want);
            if (e != hipSuccess) pl->eval_stage.reset();
            HIP_TRY(e);
        }
    }
    char *stage = pl->eval_stage.get() + pl->eval_cursor;
    char *hstage = pl->eval_host.get() + pl->eval_cursor;
    pl->eval_cursor += bytes;
    pl->eval_stream = s;
    pl->eval_pending = true;
    for (int f = 0; f < nfact; ++f)
        memcpy(hstage + tables_at + offs[f] * 8, factors[f0 + f].host, (size_t)elems[f] * (factors[f0 + f].dtype == JTP_F32 ? 4 : 8));
    if (!fvars.empty()) memcpy(hstage + fvars_at, fvars.data(), fvars.size() * sizeof(JtEvalVar));
    std::vector<int> grid((size_t)nlists, 0);
    for (int k = 0; k < nlists; ++k) {
        memcpy(hstage + task_at[k], tasks[k].data(), tasks[k].size() * sizeof(JtEvalTask));
        int32_t *bs = reinterpret_cast<int32_t *>(hstage + blk_at[k]);
        int64_t at = 0;
        for (size_t t = 0; t < tasks[k].size(); ++t) {
            bs[t] = (int32_t)at;
            at += (tasks[k][t].n_rows + JT_EVAL_ROWS - 1) / JT_EVAL_ROWS;
        }
        bs[tasks[k].size()] = (int32_t)at;
        if (at > INT32_MAX) return set_err(JTP_EUNSUPPORTED, "too many rows in one evaluate call");
        grid[k] = (int)at;
    }
    HIP_TRY(hipMemcpyAsync(stage, hstage, bytes, hipMemcpyHostToDevice, s));
    const int lds = lds_doubles * 8;
    for (int k = 0; k < nlists; ++k) {
        if (grid[k] == 0) continue;
        const JtEvalTask *dt = reinterpret_cast<const JtEvalTask *>(stage + task_at[k]);
        const int32_t *bs = reinterpret_cast<const int32_t *>(stage + blk_at[k]);
        const JtEvalVar *fvp = reinterpret_cast<const JtEvalVar *>(stage + fvars_at);
        if (k >= npass) hipLaunchKernelGGL((jt_eval_batch<double>), dim3(grid[k]), dim3(256), lds, s, dt, bs, (int)tasks[k].size(), fvp, (const char *)(stage + tables_at), b.fix);
        else if (hp.dtype == JTP_F32) hipLaunchKernelGGL((jt_eval_batch<float>), dim3(grid[k]), dim3(256), lds, s, dt, bs, (int)tasks[k].size(), fvp, (const char *)(stage + tables_at), (float *)b.psi);
        else hipLaunchKernelGGL((jt_eval_batch<double>), dim3(grid[k]), dim3(256), lds, s, dt, bs, (int)tasks[k].size(), fvp, (const char *)(stage + tables_at), (double *)b.psi);
    }
    HIP_TRY(hipGetLastError());
    return JTP_OK;                        // (the caller's tables were copied to pinned memory above)
}

int jtp_set_potential_product(jtp_plan *pl, int32_t batch, int32_t clique, int32_t n_factors, const jtp_factor *factors) {
    if (n_factors < 0 || (n_factors > 0 && !factors)) return set_err(JTP_EINVAL, "bad factor list");
    const int32_t off[2] = {0, n_factors};
    return jtp_set_potential_products(pl, batch, 1, &clique, off, factors);
}

int jtp_fill_synthetic(jtp_plan *pl, int32_t batch, uint64_t seed, const double *scale) {
    int rc = check_ready(pl, batch);
    if (rc) return rc;
    rc = check_writable(pl, batch);
    if (rc) return rc;
    pl->psi_dirty = true;
    HostPlan &hp = pl->hp;
    HIP_TRY(hipSetDevice(hp.device));
    hipStream_t s = pl->streams[batch % pl->streams.size()];
    BatchBuffers &b = pl->bufs[batch];
    for (int c = 0; c < hp.n_cliques; ++c) {
        if (!(hp.pn[c].owner == hp.rank || hp.pn[c].owner == hp.n_ranks)) continue;
        if (hp.pn[c].unit && hp.pn[c].stat < 0) continue;          // all ones, nothing stored
        const JtPackDesc &d = hp.pn[c].unit ? hp.stat_pack[c] : hp.pack[c];
        const uint64_t key = host_splitmix64(seed * 0x100000001B3ull + (uint64_t)c);
        const double sc = scale ? scale[c] : 1.0;
        const int grid = grid_1d(d.phys_elems);
        if (hp.pn[c].unit)       // (the static table: the same counter-based values over the covered shape)
            hipLaunchKernelGGL((jt_pack<double, double, 1>), dim3(grid), dim3(256), 0, s, d, (const double *)nullptr, b.fix, key, sc);
        else if (hp.dtype == JTP_F32)
            hipLaunchKernelGGL((jt_pack<float, float, 1>), dim3(grid), dim3(256), 0, s, d, (const float *)nullptr, (float *)b.psi, key, sc);
        else
            hipLaunchKernelGGL((jt_pack<double, double, 1>), dim3(grid), dim3(256), 0, s, d, (const double *)nullptr, (double *)b.psi, key, sc);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    return JTP_OK;
}

// ------------------------------------------------------------------------------------------ evidence

int jtp_set_evidence(jtp_plan *pl, int32_t batch, int32_t n, const int32_t *var_ids, const int32_t *states) {
    int rc = check_ready(pl, batch);
    if (rc) return rc;
    HostPlan &hp = pl->hp;
    if (n < 0 || (n > 0 && (!var_ids || !states))) return set_err(JTP_EINVAL, "null argument");
    BatchBuffers &b = pl->bufs[batch];
    std::vector<uint32_t> ev(2 * hp.pn.size(), 0u);
    std::vector<char> seen(hp.n_vars, 0);
    for (int i = 0; i < n; ++i) {
        const int v = var_ids[i];
        if (v < 0 || v >= hp.n_vars) return set_err(JTP_EINVAL, "evidence %d: variable %d out of range", i, v);
        if (states[i] < 0 || states[i] >= hp.card[v]) return set_err(JTP_EINVAL, "evidence %d: state %d of variable %d (cardinality %d)", i, states[i], v, hp.card[v]);
        if (seen[v]) return set_err(JTP_EINVAL, "variable %d observed twice", v);
        seen[v] = 1;
        // hard evidence is slicing: the mask goes into EVERY clique that contains the variable, so that no pass ever uses an
        // entry that contradicts it - such an entry may hold inf or NaN, and a message that is exactly 0 there does not undo that
        // (0 x inf).  Every rank fills the same table; a rank's kernels read the rows of the cliques it runs.
        bool held = false;
        for (int c = 0; c < hp.n_cliques; ++c) {
            const PNode &p = hp.pn[c];
            for (size_t j = 0; j < p.vars.size(); ++j)
                if (p.vars[j] == v) {
                    ev[2 * c] |= ((1u << p.nb[j]) - 1u) << p.pos[j];
                    ev[2 * c + 1] |= (uint32_t)states[i] << p.pos[j];
                    held = true;
                }
        }
        if (!held) return set_err(JTP_EINVAL, "variable %d is in no clique", v);
    }
    HIP_TRY(hipSetDevice(hp.device));
    hipStream_t s = pl->streams[batch % pl->streams.size()];
    HIP_TRY(hipStreamSynchronize(s));                      // a propagate in flight may still read the old table
    if (!b.ev) {                                            // (multi-set plans: a slice of ev_all, set at plan creation)
        HIP_TRY(pl->set_mem[batch].ev.alloc(ev.size()));
        b.ev = pl->set_mem[batch].ev.get();
    }
    HIP_TRY(hipMemcpy(b.ev, ev.data(), ev.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    b.ev_any = n > 0;
    // (the host's copy, by variable: jtp_map uploads the rows of the sets it works on)
    if (pl->ev_obs.empty()) pl->ev_obs.assign((size_t)hp.n_batch * (size_t)hp.n_vars, -1);
    std::fill_n(pl->ev_obs.begin() + (size_t)batch * (size_t)hp.n_vars, (size_t)hp.n_vars, -1);
    for (int i = 0; i < n; ++i) pl->ev_obs[(size_t)batch * (size_t)hp.n_vars + (size_t)var_ids[i]] = states[i];
    if (pl->multiset) {
        // a group of evidence sets may sum the elements of a vector before the message product on a clique while none of ITS
        // sets observes a variable on that clique's element bits (JtTask::esum_groups; bit b stands for the groups g = b mod 64)
        const int iset = pl->set0 + batch;                       // the set's place in the allocation (group 0: evidence-free sets)
        std::copy(ev.begin(), ev.end(), pl->ev_host.begin() + (size_t)iset * pl->ev_stride);
        if (pl->set0) pl->act_dirty = true;                       // (the tasks' active lists follow the evidence: rebuilt by the next propagate)
        const uint32_t emask = (1u << hp.EB) - 1u;
        const int bit = (iset / JT_MSETS) & 63;
        std::vector<char> on_e(hp.pn.size(), 0);
        const size_t nsets = pl->ev_host.size() / pl->ev_stride;
        for (size_t sidx = 0; sidx < nsets; ++sidx) {
            if ((int)((sidx / JT_MSETS) & 63) != bit) continue;
            for (size_t p = 0; p < hp.pn.size(); ++p)
                if (pl->ev_host[sidx * pl->ev_stride + 2 * p] & emask) on_e[p] = 1;
        }
        const bool always = hp.knobs.esum_always != 0;             // (timing experiment: wrong results)
        for (size_t t = 0; t < hp.tasks.size(); ++t) {
            JtTask &tk = hp.tasks[t];
            if (tk.kind != 0 || !(tk.esum & 1)) continue;
            const uint64_t want = (on_e[tk.pnode] && !always) ? tk.esum_groups & ~(1ull << bit) : tk.esum_groups | (1ull << bit);
            if (want != tk.esum_groups) {
                tk.esum_groups = want;
                tk.esum = 1 | (want == ~0ull ? 2 : 0);
                pl->esum_dirty = true;                               // uploaded in one copy by the next jtp_propagate
            }
        }
    }
    return JTP_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------ active lists

// Multi-set plans with an evidence-free set (round 6): which evidence sets every task serves.  The upward message of a clique below
// which a set observes NOTHING is the evidence-free one, whatever the set observes elsewhere; with 16 observations per set on the
// width-20 tree that is four collect tasks in five, per SET - round 5 skipped a task only where all eight sets of a fixed group
// agreed, one in three.  So the sets of a workgroup are no longer "group g" but entries 8 g .. 8 g + 7 of the TASK's list:
//   collect task of clique c (and its reduce task): arena slot 0 - the evidence-free set - and every caller's set with an observed
//     variable in the subtree below c;
//   downward task: every caller's slot (and the padding slots behind them, which exist: the last group as before).
// A consumer stages an upward message of slot s from s's own arena where s is on the producer's list, from slot 0 where it is not
// (JtFlow::skip = member) - and so does the read-out (readout_redirect): nobody copies slot 0's messages into the other sets' arenas
// (round 5 and the first form of this round did, behind every propagate: 7 % of a 64-set step).  The entries of a (task, slot) off the
// lists stay "unwritten" in both arena halves; those of a pair that LEAVES a list are set back to that, once, here.
int rebuild_active(jtp_plan *pl, hipStream_t s) {
    const HostPlan &hp = pl->hp;
    const int cap = pl->n_groups * JT_MSETS, set0 = pl->set0, S = hp.n_batch;
    const size_t nt = hp.tasks.size(), np = hp.pn.size();
    const std::vector<uint8_t> was = pl->member_host;       // the lists of the last propagate (empty: none yet)
    pl->member_host.assign(nt * cap, 0);
    pl->act_ids_host.assign(nt * cap, 0);
    pl->act_n_host.assign(nt, 0);
    pl->esum_oct_host.assign(nt * (size_t)pl->n_groups, 0);
    // below[slot * np + p]: the set in that slot observes a variable hosted by clique p or by a clique below it
    std::vector<uint8_t> below((size_t)cap * np, 0);
    std::vector<int> order(np);
    for (size_t p = 0; p < np; ++p) order[p] = (int)p;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return hp.pn[a].depth > hp.pn[b].depth; });
    for (int slot = set0; slot < set0 + S; ++slot) {
        uint8_t *bl = &below[(size_t)slot * np];
        const uint32_t *ev = &pl->ev_host[(size_t)slot * pl->ev_stride];
        for (size_t p = 0; p < np; ++p) bl[p] = ev[2 * p] != 0;
        for (int p : order)
            if (bl[p] && hp.pn[p].parent >= 0) bl[hp.pn[p].parent] = 1;
    }
    auto put = [&](int t, const std::vector<uint16_t> &list) {
        if (t < 0) return;
        pl->act_n_host[t] = (int32_t)list.size();
        for (size_t j = 0; j < list.size(); ++j) {
            pl->act_ids_host[(size_t)t * cap + j] = list[j];
            pl->member_host[(size_t)t * cap + list[j]] = 1;
        }
    };
    std::vector<uint16_t> everyone;
    for (int slot = set0; slot < cap; ++slot) everyone.push_back((uint16_t)slot);
    // What leaves a list is reset: the entries of a (collect task, slot) that was on the task's list for the last propagate and is not
    // now hold that propagate's values - in the halves' turn the task would find them "written" when the slot comes back (its reduce
    // task sums the partial copies it finds without a marker).  Both halves of such messages, partial copies included, are marked
    // "unwritten" ONCE, here; entries of pairs that stay off the lists are never read (consumers and read-out go to slot 0) nor written.
    std::vector<JtFanout> fan;
    auto reset = [&](int64_t off, int64_t count, const std::vector<uint16_t> &slots) {
        for (size_t i = 0; i < slots.size(); i += JT_MSETS) {
            JtFanout f;
            memset(&f, 0, sizeof f);
            f.off = off, f.count = (int32_t)count, f.flags = JT_FANOUT_RESET;
            for (int j = 0; j < JT_MSETS; ++j) f.slot[j] = i + j < slots.size() ? slots[i + j] : (uint16_t)0xffffu;
            fan.push_back(f);
        }
    };
    for (size_t p = 0; p < np; ++p) {
        const PNode &pn = hp.pn[p];
        if (pn.collect_task >= 0) {
            std::vector<uint16_t> list(1, (uint16_t)0), left;
            for (int slot = set0; slot < set0 + S; ++slot) {
                const bool on = below[(size_t)slot * np + p] != 0;
                if (on) list.push_back((uint16_t)slot);
                else if (!was.empty() && was[(size_t)pn.collect_task * cap + slot]) left.push_back((uint16_t)slot);
            }
            put(pn.collect_task, list);
            const PSep &sp = hp.ps[pn.psep];
            put(sp.up_red_task, list);
            if (!left.empty()) {
                reset(sp.up_roff, ((int64_t)sp.up_rnpart) << sp.nbits, left);
                if (sp.up_red_task >= 0) reset(sp.up_off, ((int64_t)sp.up_npart) << sp.nbits, left);
            }
        }
    }
    for (const PSep &sp : hp.ps) {
        put(sp.dn_task, everyone);
        put(sp.dn_red_task, everyone);
    }
    const uint32_t emask = (1u << hp.EB) - 1u;
    for (size_t t = 0; t < nt; ++t) {
        const JtTask &tk = hp.tasks[t];
        if (tk.kind != 0 || !(tk.esum & 1)) continue;
        const int n = pl->act_n_host[t];
        for (int g = 0; g * JT_MSETS < n; ++g) {
            bool free_e = true;
            for (int j = g * JT_MSETS; j < std::min(n, (g + 1) * JT_MSETS); ++j)
                if (pl->ev_host[(size_t)pl->act_ids_host[t * cap + j] * pl->ev_stride + 2 * tk.pnode] & emask) free_e = false;
            pl->esum_oct_host[t * (size_t)pl->n_groups + g] = (free_e || hp.knobs.esum_always) ? 1 : 0;
        }
    }
    HIP_TRY(pl->d_fanout.reserve(fan.size()));
    HIP_TRY(hipMemcpyAsync(pl->d_member.get(), pl->member_host.data(), pl->member_host.size(), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(pl->d_act_ids.get(), pl->act_ids_host.data(), pl->act_ids_host.size() * sizeof(uint16_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(pl->d_act_n.get(), pl->act_n_host.data(), pl->act_n_host.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(pl->d_esum_oct.get(), pl->esum_oct_host.data(), pl->esum_oct_host.size(), hipMemcpyHostToDevice, s));
    if (!fan.empty()) HIP_TRY(hipMemcpyAsync(pl->d_fanout.get(), fan.data(), fan.size() * sizeof(JtFanout), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                    // (the sources are host vectors)
    pl->n_fanout = (int)fan.size();
    pl->act_dirty = false;
    if (pl->n_fanout > 0) {
        JtFlow fl;
        memset(&fl, 0, sizeof fl);
        fl.set_stride = pl->set_stride;
        fl.oth_off = pl->half;                                      // (the second half starts here: the pass marks both)
        hipLaunchKernelGGL(jt_multi_fanout, dim3(pl->n_fanout), dim3(256), 0, s, pl->d_fanout.get(), pl->msg_all.get(), fl);
        HIP_TRY(hipGetLastError());
        // (the marks cover the partial copies of chunks that do not exist, which nobody writes again: set back to their zeros)
        if (pl->d_init[0] || pl->d_init[1])
            if (int rc = zero_padding(pl, pl->msg_all.get(), pl->n_groups * JT_MSETS, s)) return rc;
    }
    return JTP_OK;
}
