/* jtprop.h - C ABI of libjtprop.so, the MI355X (gfx950) sum-product engine that replaces
 * the message-passing hot path of jluttine/junction-tree.
 *
 * Boundary: the reference's per-call seam is
 *     SumProduct(einsum).einsum(...)                 junctiontree/sum_product.py:22-43
 * which is one host round trip per einsum and too fine for a GPU.  The device boundary is
 * therefore `compute_beliefs` granularity - whole junction tree in, all beliefs out:
 *     compute_beliefs(tree, potentials, clique_vars)  junctiontree/computation.py:37-246
 *     JunctionTree.propagate(xs)                      junctiontree/junctiontree.py:297-331
 * Each entry point below names the reference lines it stands in for.
 *
 * Conventions: plain C, no exceptions across the boundary.  Every function returning int
 * returns JTP_OK (0) or a negative JTP_E* code; jtp_last_error() then holds a message
 * (thread local).  Host arrays are C-order in the node's own variable order exactly as the
 * reference passes numpy arrays (README.md:22-41).  A plan is not thread safe; distinct
 * plans are independent.  All device work of a plan runs on the plan's own HIP stream.
 */
#ifndef JTPROP_H
#define JTPROP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define JTP_OK 0
#define JTP_EINVAL (-1)     /* bad argument / malformed tree (Python: ValueError)        */
#define JTP_EHIP (-2)       /* HIP runtime error, or no GPU (Python: RuntimeError)      */
#define JTP_ECOMM (-3)      /* RCCL error                                               */
#define JTP_ENOMEM (-4)     /* device or host allocation failed                         */
#define JTP_EUNSUPPORTED (-5) /* structure outside engine limits (e.g. table > 2^31)    */

#define JTP_F32 0           /* clique tables stored as float  (messages are always f64) */
#define JTP_F64 1           /* clique tables stored as double                           */

#define JTP_PLAN_ONLY 1u    /* jtp_tree_desc.flags: plan on the host only, touch no GPU  */
#define JTP_KEEP_ROOT 4u    /* do not re-root the tree at its centre (default: re-root when n_ranks == 1;
                               beliefs do not depend on the root, the number of levels does)     */
#define JTP_SPLIT_VARIANTS 2u /* one launch per (level, neighbour count) instead of per level:
                               profiling aid, attributes device time to each clique shape   */

#define JTP_LEVEL_LAUNCHES 8u /* one launch per tree level instead of the default one per phase, whose
                               workgroups wait for the message entries they need (dataflow)   */

#define JTP_FLOW_TICKETS 16u /* dataflow launches: workgroups draw their place in the block list from an
                               atomic counter instead of relying on in-order workgroup dispatch     */

#define JTP_SHARE_POTENTIALS 32u /* the n_batch evidence sets read ONE set of clique potentials (set through
                               evidence set 0) and differ by their evidence (jtp_set_evidence): BASELINE
                               config 5 without 512 copies of the tables, and with the concurrently running
                               sets finding each other's table reads in the last-level cache             */

#define JTP_MULTISET 64u    /* with JTP_SHARE_POTENTIALS: evidence sets are processed EIGHT at a time by one pass over the
                               shared clique tables (kernel jt_multi_flow): a table row is read from HBM once per
                               group of sets instead of once per set.  No belief tables are kept: clique beliefs and
                               marginals are formed on demand from the shared tables and the set's final messages;
                               jtp_propagate always runs all evidence sets of the plan                        */

#define JTP_NO_COMPACT 128u /* store every clique table padded to powers of two in every variable (round-1 layout).  By
                               default the rows above the thread part are stored at the true cardinalities         */

#define JTP_SCALED 256u     /* overflow-safe propagate: every message is divided by a power of two right after it is produced
                               (its largest entry then lies in [1, 2)), the exponents are kept per evidence set, and the
                               read-out reports them: jtp_get_log2_scale, jtp_get_log_z.  Powers of two commute exactly with
                               every multiply and add downstream, so - absent underflow, overflow and subnormals - a scaled
                               propagate gives the unscaled tables bit for bit, up to a known exponent per node.  Such a plan
                               always launches per tree level (as JTP_LEVEL_LAUNCHES) with one small launch per level and phase
                               on top; refused (JTP_EUNSUPPORTED) with JTP_MULTISET and with n_ranks > 1                    */

typedef struct jtp_plan jtp_plan;

/* Structure of one junction tree.  Mirrors the reference's data model
 * (junctiontree/junctiontree.py:141-189, 283-291; README.md:50-77): a node list that is the
 * concatenation of maximal cliques (nodes 0..n_cliques-1) and separators (nodes
 * n_cliques..n_nodes-1), each node a list of variables, plus the tree given here in flat
 * parent form instead of the nested list (the Python layer flattens it). */
typedef struct jtp_tree_desc {
    int32_t struct_size;            /* sizeof(jtp_tree_desc), for ABI versioning             */
    int32_t n_vars;                 /* number of distinct variables                          */
    const int32_t *var_card;        /* [n_vars] cardinality of each variable (>= 1)          */
    int32_t n_cliques;              /* number of maximal cliques (>= 1)                      */
    int32_t n_nodes;                /* n_cliques + number of separators (= 2*n_cliques - 1)  */
    const int32_t *node_var_off;    /* [n_nodes+1] CSR offsets into node_var_ids             */
    const int32_t *node_var_ids;    /* variable ids of each node in its host axis order      */
    const int32_t *parent_clique;   /* [n_cliques] parent clique, -1 for the root            */
    const int32_t *parent_sep;      /* [n_cliques] node index of the separator to the parent */
    int32_t dtype;                  /* JTP_F32 or JTP_F64                                    */
    int32_t device;                 /* HIP device ordinal used by this process               */
    int32_t n_batch;                /* independent evidence sets sharing the structure (>=1) */
    int32_t n_ranks;                /* processes sharing the tree (1 = single GPU)           */
    int32_t rank;                   /* this process                                          */
    const int32_t *clique_owner;    /* [n_cliques] owning rank, or NULL (all rank 0)         */
    uint32_t flags;                 /* JTP_PLAN_ONLY | JTP_SPLIT_VARIANTS | JTP_KEEP_ROOT | JTP_LEVEL_LAUNCHES | ... */
    int32_t lds_budget;             /* bytes of LDS per workgroup the planner may use, 0=default */
    int32_t block_log2;             /* log2 of target elements per workgroup, 0 = automatic  */
    int32_t layout_policy;          /* bit order of the clique tables: 0 = chosen per clique (2 or 3 by the size of
                                       its messages), 1 = host axis order, 2 = variables of the fewest messages
                                       lowest (least message traffic), 3 = message variables in the thread part
                                       (cheapest reduction)                                   */
    /* Which variables of each clique its potential DEPENDS on (NULL: all of them).  The reference leaves every
     * variable of a clique that none of its assigned factors covers as a length-1 axis and never materialises it
     * (junctiontree/junctiontree.py:52-61, evaluate :203-226).  A clique that lists only some of its variables here
     * keeps NO full-size table on the device: its potential is stored at the covered shape and broadcast inside the
     * passes, its belief is formed on demand (jtp_get_belief / jtp_get_marginals), a clique that lists none is all
     * ones and stores nothing.  jtp_set_potential / jtp_set_potential_product(s) of such a clique take arrays whose
     * axes of the other variables have length 1.  (The engine may still materialise a clique whose covered part is
     * most of it; jtp_plan_describe says which.)  Ignored by JTP_MULTISET plans. */
    const int32_t *cover_off;       /* [n_cliques+1] CSR offsets into cover_ids, or NULL          */
    const int32_t *cover_ids;       /* covered variable ids of each clique (a subset of its own)  */
    /* The marginals the caller asks for after every propagate (round 6; 0 / NULL: none named): the list jtp_get_marginals will be
     * called with - per request a clique and the variables to keep, in that order.  JunctionTree.propagate returns factor marginals
     * only (junctiontree/junctiontree.py:264-274, 327-331), so the list is known when the plan is made.  Requests on cliques that keep
     * no table are then formed INSIDE the propagate's launch - tasks of their own on the level of the clique's downward messages,
     * filling slots the dependent levels leave idle - and a jtp_get_marginals call with exactly this list only unpacks them.  A hint:
     * any other list, an evidence set that observes something, or a plan whose launches cannot take such tasks is served as before. */
    int32_t fold_n;
    int32_t fold_pad;
    const int32_t *fold_cliques;    /* [fold_n] clique of each request                            */
    const int32_t *fold_var_off;    /* [fold_n+1] CSR offsets into fold_var_ids                   */
    const int32_t *fold_var_ids;    /* the variables each request keeps                           */
} jtp_tree_desc;

/* Counters of the last jtp_propagate (device time needs jtp_set_profiling(plan, 1)). */
typedef struct jtp_stats {
    int32_t struct_size;
    int32_t n_launches;             /* kernel launches per propagate                         */
    int32_t n_messages;             /* directed tree edges processed = 2*(n_cliques-1)       */
    int32_t n_tasks;
    double  algorithmic_bytes;      /* SURVEY.md 8d definition, this rank's share            */
    double  collect_ms;             /* device time of the collect phase (profiling on)       */
    double  distribute_ms;          /* device time of the distribute phase                   */
    double  kernel_ms[32];          /* device time per kernel variant, mean per propagate    */
    double  kernel_bytes[32];       /* algorithmic bytes processed per kernel variant        */
    int32_t kernel_launches[32];    /* launches per kernel variant                           */
    int32_t flow_fallbacks;         /* dataflow launches that timed out and were re-run per level (expected 0) */
    int32_t launch_mode;            /* of the last jtp_propagate: 0 = one launch per tree level, 1 = dataflow launches in
                                       blockIdx order (the default), 2 = dataflow launches in ticket order            */
    int32_t tickets_used;           /* propagates (counted per evidence set) since plan creation that ran in ticket order */
    int32_t flow_propagates;        /* propagates (per evidence set) since plan creation that ran as dataflow launches  */
    double  device_bytes;           /* bytes the plan held when jtp_plan_create returned: every buffer, counted as allocated */
    int32_t storage_dtype;          /* JTP_F32 / JTP_F64 the clique tables are stored as: a float32 request is made with float64
                                       tables where the float32 layout cannot be planned (sub-boxes beyond the LDS of a CU) */
    int32_t foreign_seen;           /* propagates since plan creation that found ANOTHER PROCESS with a dataflow propagate in flight
                                       on the device (a shared-memory board, /dev/shm/jtprop_flight_<PCI bus id>) and therefore ran
                                       in ticket order - counted in tickets_used as well                                    */
    double  f64_flops;              /* multi-set plans: float64 operations of one propagate (multiplications and additions of the
                                       element loop, a fused multiply-add counted as two; conversions, index arithmetic, staging and
                                       epilogues not counted): the kernel jt_multi_flow is bound by them, not by HBM; else 0 */
    double  f64_insts;              /* ... and the float64 vector instructions (per lane) that stands for: a multiplication
                                       occupies the pipe as long as a fused multiply-add does                              */
    double  algorithmic_bytes_full; /* algorithmic bytes with EVERY clique counted at its full shape, read in both passes and its
                                       belief written (SURVEY.md 8d to the letter).  `algorithmic_bytes` counts a clique that keeps
                                       no table (jtp_tree_desc.cover_*) as what its potential is: the table over the covered
                                       variables, read once per pass, no belief                                            */
    double  fixed_bytes;            /* bytes of the static tables of such cliques (per evidence set, or shared)            */
    int32_t n_unit_cliques;         /* cliques of the caller's tree that keep no table on the device                       */
    int32_t n_static_tables;        /* ... of which hold factors: their product is a static table over the covered variables */
    int32_t flight_board;           /* 1: this process publishes its in-flight dataflow propagates on the device's shared-memory board
                                       (/dev/shm/jtprop_flight_<PCI bus id>) and sees other processes'; 0: the board could not be opened
                                       (another user's file, no /dev/shm): other PROCESSES on the device are then only noticed by the
                                       2 s time-out; -1: no dataflow propagate has asked for it yet                              */
    int32_t lean_refused;           /* 1: the description named covered variables (cover_*) but the plan that keeps no table for the
                                       uncovered part was refused (JTP_EUNSUPPORTED: a static table's sub-boxes beyond LDS, ...) and
                                       the tree was planned with EVERY table materialised - on lattices many times the device
                                       memory; the reason is the "lean_refused" string of jtp_plan_describe                      */
} jtp_stats;

/* ---- lifetime ------------------------------------------------------------------------- */

/* Compile a tree into a device plan: variable->bit layout of every table, level schedule
 * of collect (computation.py:47-96) and distribute (:140-224), message buffers, kernel task
 * tables, and (n_ranks > 1) the separator exchange schedule.  Replaces the per-call label
 * bookkeeping of sum_product.py:22-43 and the recursion of computation.py:227-243. */
int jtp_plan_create(const jtp_tree_desc *desc, jtp_plan **out);
void jtp_plan_destroy(jtp_plan *plan);

/* JSON description of the plan (layouts, tasks, launches, exchange schedule).  The string is
 * owned by the plan and valid until the plan is destroyed.  Used by tests and DESIGN.md. */
const char *jtp_plan_describe(jtp_plan *plan);

/* ---- data in -------------------------------------------------------------------------- */

/* Upload the potential of clique `node` (0 <= node < n_cliques) for evidence set `batch`.
 * `host` is a C-order array over the node's variables; `shape[i]` is the actual length of
 * axis i: the variable's cardinality, or 1 to broadcast along it (numpy semantics the
 * reference relies on, junctiontree.py:52-61).  `host_dtype` is JTP_F32 or JTP_F64.
 * Stands in for `np.copy(p)` of computation.py:245.  Separator potentials are never
 * uploaded: the reference overwrites them before use.
 * LIFETIME OF `host`: the call enqueues the copy on the plan's stream and does NOT wait for it.  From pageable
 * memory the HIP runtime has staged the caller's bytes when the call returns, so the array may be changed or freed at
 * once.  From PAGE-LOCKED memory (jtp_host_alloc, hipHostMalloc, hipHostRegister) the copy is truly asynchronous:
 * the caller must keep the array alive and unmodified until the next jtp_sync (or any read-out call, which
 * synchronises the evidence set's stream) of this plan.  jtp_set_potential_product copies its tables before it
 * returns and has no such rule. */
int jtp_set_potential(jtp_plan *plan, int32_t batch, int32_t node, const void *host,
                      const int64_t *shape, int32_t host_dtype);

/* One factor table handed to jtp_set_potential_product. */
typedef struct jtp_factor {
    const void *host;               /* C-order table over `var_ids`                           */
    int32_t n_vars;
    int32_t dtype;                  /* JTP_F32 or JTP_F64                                     */
    const int32_t *var_ids;         /* [n_vars] variables (a subset of the clique's)          */
    const int64_t *shape;           /* [n_vars] actual axis lengths: cardinality, or 1        */
} jtp_factor;

/* Clique potential = product of the factor tables assigned to the clique, formed ON THE DEVICE
 * in the clique's layout: CliqueGraph.evaluate for one clique (junctiontree.py:203-226, helper
 * einsum :34-80).  Only the factor tables cross PCIe; variables no factor covers are constant
 * axes (the reference leaves them length 1).  n_factors = 0 gives all ones. */
int jtp_set_potential_product(jtp_plan *plan, int32_t batch, int32_t clique, int32_t n_factors,
                              const jtp_factor *factors);

/* The same for a LIST of cliques - all of CliqueGraph.evaluate (junctiontree.py:203-226: one helper einsum per clique)
 * as ONE host-to-device copy of every factor table and ONE kernel launch over all the listed cliques.  Clique cliques[i]
 * receives the product of factors[factor_off[i] .. factor_off[i+1]); a clique may be listed with no factors (all ones),
 * no clique may be listed twice (JTP_EINVAL).
 * The tables are copied before the call returns.  A caller that knows which factor tables changed since the last call
 * lists only their cliques (junctiontree_amd/junctiontree.py does). */
int jtp_set_potential_products(jtp_plan *plan, int32_t batch, int32_t n_cliques, const int32_t *cliques,
                               const int32_t *factor_off, const jtp_factor *factors);

/* Fill every clique potential on the device with the counter-based synthetic values of
 * junctiontree_amd/synthetic.py: psi[i] = (0.5 + u(seed, node, i)) * scale[node], i the
 * C-order host index.  For benchmarks (no host transfer). */
int jtp_fill_synthetic(jtp_plan *plan, int32_t batch, uint64_t seed, const double *scale);

/* Hard evidence of one evidence set: variable var_ids[i] is observed in state states[i].  Replaces the
 * set's previous evidence (n = 0 clears it).  Hard evidence is slicing, as apply_evidence of the reference
 * defines it (computation.py:11-34): in EVERY clique that contains the variable the entries that contradict
 * the evidence are never used - whatever they hold, inf and NaN included - and nothing is rewritten.  On
 * finite tables that equals a one-hot indicator multiplied into one such clique (the equivalence
 * tests/test_computation.py:411-459 of the reference demonstrates).  Takes effect at the next jtp_propagate. */
int jtp_set_evidence(jtp_plan *plan, int32_t batch, int32_t n, const int32_t *var_ids, const int32_t *states);

/* ---- compute -------------------------------------------------------------------------- */

/* Collect then distribute for evidence sets [batch_begin, batch_end): the body of
 * compute_beliefs (computation.py:227-243).  Asynchronous; pair with jtp_sync. */
int jtp_propagate(jtp_plan *plan, int32_t batch_begin, int32_t batch_end);
int jtp_sync(jtp_plan *plan);

/* ---- data out ------------------------------------------------------------------------- */

/* Belief of `node` (clique: psi * all incoming messages, computation.py:216-224;
 * separator: up * down, computation.py:210), written to `host` in the node's host axis
 * order at full cardinalities, as `host_dtype`.  Unnormalised, sums to Z. */
int jtp_get_belief(jtp_plan *plan, int32_t batch, int32_t node, void *host, int32_t host_dtype);

/* Marginal of clique `clique`'s belief onto `out_vars` (a subset of its variables, in the
 * requested order), as doubles: CliqueGraph.marginalize for one factor
 * (junctiontree.py:264-274). */
int jtp_get_marginal(jtp_plan *plan, int32_t batch, int32_t clique, const int32_t *out_vars,
                     int32_t n_out, double *host);

/* Many marginals in one go: all of CliqueGraph.marginalize (junctiontree.py:229-274, one
 * einsum per factor) as ONE kernel launch over every requested clique, one conversion launch
 * and one device-to-host copy.  Request i asks clique `cliques[i]` for the variables
 * var_ids[var_off[i] .. var_off[i+1]) (that axis order) and receives them at host + out_off[i]
 * (doubles, C order).  The device tables of a request list are kept with the plan, so asking for
 * the same list again (every propagate of one model does) costs no planning. */
int jtp_get_marginals(jtp_plan *plan, int32_t batch, int32_t n, const int32_t *cliques,
                      const int32_t *var_off, const int32_t *var_ids, const int64_t *out_off,
                      double *host);

/* Z = sum of the root belief (the value the reference computes and drops,
 * computation.py:90-96).  On a JTP_SCALED plan: ldexp(sum of the scaled root belief, E_root) - which may be inf or 0 where
 * Z lies outside float64; jtp_get_log_z always has it. */
int jtp_get_z(jtp_plan *plan, int32_t batch, double *z);

/* JTP_SCALED plans: every table the read-out returns for `node` (clique or separator: jtp_get_belief, jtp_get_marginal(s)) of the
 * last propagate of evidence set `batch` is the true table times 2^-E; *e = E.  0 on plans without the flag. */
int jtp_get_log2_scale(jtp_plan *plan, int32_t batch, int32_t node, int64_t *e);

/* log|Z| = log|sum of the root belief| + E_root ln 2, and the sign of Z in {-1, 0, 1} (the reference allows signed values;
 * sign 0: *log_abs_z = -inf).  Works on every plan (E = 0 without JTP_SCALED). */
int jtp_get_log_z(jtp_plan *plan, int32_t batch, double *log_abs_z, int32_t *sign);

/* n_samples joint draws from the beliefs of the last propagate of evidence set `batch`:
 * states[i * n_vars + v] = state of variable v in sample i (-1: the sample met a slice without mass).
 * One root-to-leaves sweep over the tree as the description gave it (parent_clique; the root is the clique whose parent is -1):
 * clique c conditions on the variables it shares with its parent clique - already drawn - and draws its other variables jointly,
 * as the inverse CDF of that slice of its belief (entries in C order over the drawn variables in the clique's host axis order,
 * summed in float64) at u = ((splitmix64(key(seed, c) + i)) >> 11) * 2^-53, key as junctiontree_amd/synthetic.py sample_uniform
 * has it.  Sample i depends on (seed, i) and the beliefs only - not on n_samples, nor on the plan's layout or launch flags - and an
 * entry that is drawn is never zero.  Observed variables (jtp_set_evidence) come out in their observed state.  Works on JTP_SCALED
 * plans as it stands (a power of two per clique cancels).
 * JTP_EUNSUPPORTED: JTP_MULTISET plans, n_ranks > 1, plans in which a clique keeps no table (cover_*).  Where a slice has a zero
 * or non-finite total, or a negative or NaN entry (evidence of probability zero, overflow), the variables that sample would have
 * drawn there, and below, are -1; the states are still copied out, the call returns JTP_EINVAL and the message names the number
 * of such (clique, sample) pairs and the first clique. */
int jtp_sample(jtp_plan *plan, int32_t batch, int32_t n_samples, uint64_t seed, int32_t *states);

/* The most probable joint assignment of every evidence set in [batch_begin, batch_end), by a max-product sweep over the clique
 * potentials on the device: states[(b - batch_begin) * n_vars + v] = state of variable v for set b (a variable of no clique: 0),
 * log_value (NULL, or [batch_end - batch_begin]) = log max_x prod_c psi_c(x) over the assignments x that agree with the set's evidence
 * (jtp_set_evidence as last called - no propagate is needed, and the beliefs and messages one left are not touched); log_value less
 * jtp_get_log_z of the set is the assignment's log posterior probability.
 * The sweep runs over the tree as the description gave it, on the schedule of jtp_sample (by depth, then clique number; K_c = the
 * variables clique c shares with its parent clique, F_c the others in host axis order, R_c = prod card(F_c)).  Upward, deepest first:
 * for every assignment k of K_c, raw_c[k] = max over r in [0, R_c) of w(k, r) = ((double)psi_c[k, r] * m_1) * m_2 ... - the children
 * of c in ascending clique number, float64, left to right - and arg_c[k] = the SMALLEST such r (C order over F_c); m_d =
 * ldexp(raw_d[k_d], -e_d), e_d = ilogb(max raw_d): every message is read divided by a power of two that puts its largest entry in
 * [1, 2), so nothing overflows whatever the depth (JTP_SCALED is not needed and changes nothing).  Entries that contradict the
 * evidence are not looked at; raw_c[k] = 0 where k does.  Downward, every clique reads arg_c at the digits the cliques above wrote.
 * log_value = log(max raw_root) + ln 2 * (sum of e_c over the other cliques).  Nothing depends on the plan's layout or launch flags:
 * equal potentials and evidence give equal states, ties included.  All sets of a chunk go through the same launches (one per depth);
 * a chunk is as many sets as keep the raw and arg tables - 12 bytes per assignment of K_c, summed over the cliques - under 64 MiB.
 * Works on plans of one set, of n_batch sets and with JTP_SHARE_POTENTIALS, float32 and float64 tables, any layout.
 * JTP_EUNSUPPORTED: JTP_MULTISET plans, n_ranks > 1, plans in which a clique keeps no table (cover_*).  A set FAILS where an entry
 * that agrees with its evidence is negative or NaN, or where a clique's largest raw entry is zero or not finite (evidence of
 * probability zero): its states are all -1, its log_value -inf; every set of the range is still written, the call returns JTP_EINVAL
 * and the message names the number of failed sets and the first. */
int jtp_map(jtp_plan *plan, int32_t batch_begin, int32_t batch_end, int32_t *states, double *log_value);

/* Max-propagation: the max-marginals of a request list for every evidence set in [batch_begin, batch_end).  A request is as in
 * jtp_get_marginals - clique cliques[i], variables V_i = var_ids[var_off[i] .. var_off[i+1]) of that clique, in that axis order (none:
 * one entry) - and its max-marginal is, for every assignment h of V_i, the largest prod_c psi_c(x) over the full assignments x that
 * agree with h and with the set's evidence:
 *     host[(b - batch_begin) * set_stride + out_off[i] + h] = that value times 2^-S   (doubles, C order; 0 where h contradicts the evidence)
 *     log2_scale[(b - batch_begin) * n + i] = S, an exponent per (set, clique)
 *     log_value (NULL, or [batch_end - batch_begin]) = what jtp_map reports for the set, bit for bit: it is the same computation.
 * The largest entry of every request table of a set times 2^S is the value of the set's most probable assignment.  No propagate is
 * needed, beliefs and messages are not touched; the evidence is what jtp_set_evidence last gave each set.
 * The sweep runs on the schedule of jtp_sample / jtp_map (by depth, then clique number; K_c = the variables clique c shares with its
 * parent clique, F_c the others in host axis order; children in ascending clique number), float64 throughout, and only entries that
 * agree with the evidence are looked at.  Upward, deepest first, jtp_map's pass as it stands: raw_c[k] = max_r ((double)psi_c[k, r] *
 * m_1) * m_2 ..., e_c = ilogb(max raw_c), m_c = ldexp(raw_c, -e_c).  Downward, shallowest first (the root has no parent message):
 * for clique c and each child d,
 *     rawdn_d[k_d] = max over the entries (k, r) of c that agree with k_d of ((psi_c[k, r] * D_c[k]) * m_d1) * m_d2 ...
 * - the parent's message D_c first (absent at the root), then the children of c in ascending clique number WITHOUT d; k_d indexed
 * as raw_d is; 0 where k_d contradicts the evidence -, f_d = ilogb(max rawdn_d), D_d = ldexp(rawdn_d, -f_d).  A request on clique c:
 *     out[h] = max over the entries of c that agree with h of ((psi_c[k, r] * D_c[k]) * m_d1) * m_d2 ...     all children of c this time.
 * The exponents are added up on the host as integers: U_d = e_d + sum of U_x over the children x of d; V_root = 0, V_d = V_c + (sum
 * of U_s over the siblings s != d) + f_d; S_c = V_c + sum of U_d over the children d of c.  A maximum is exact whatever the order and
 * the order of the multiplications is fixed above, so nothing depends on the plan's layout, compaction, root or launch flags, nor on
 * how r is cut into segments or the sets into chunks: equal potentials and evidence give bit-equal tables and exponents.
 * All sets of a chunk go through the same launches - jtp_map's upward ones, one per depth over the downward messages into that depth,
 * one over all requests -; a chunk is as many sets as keep the work area (raw and arg tables, down tables, segment results, maxima,
 * evidence rows, request outputs) under 64 MiB.  The records of the last request list are kept with the plan.  A task per (clique,
 * child) multiplies all but one of the clique's incoming messages into every entry: the downward pass is quadratic in the children
 * of one clique.
 * Works where jtp_map works: plans of one set, of n_batch sets and with JTP_SHARE_POTENTIALS, float32 and float64 tables, any layout.
 * JTP_EUNSUPPORTED: JTP_MULTISET plans, n_ranks > 1, plans in which a clique keeps no table (cover_*).  JTP_EINVAL: a bad range, a
 * request variable that is not in its clique or is listed twice, entries that do not fit set_stride, null arguments.  A set FAILS
 * where an entry that agrees with its evidence is negative or NaN, or where a maximum that feeds a message (max raw_c, max rawdn_d) is
 * zero or not finite (evidence of probability zero): its tables are all 0, its exponents 0, its log_value -inf; every set of the range
 * is still written, the call returns JTP_EINVAL and the message names the number of failed sets and the first. */
int jtp_max_marginals(jtp_plan *plan, int32_t batch_begin, int32_t batch_end, int32_t n, const int32_t *cliques, const int32_t *var_off,
                      const int32_t *var_ids, const int64_t *out_off, int64_t set_stride, double *host, int64_t *log2_scale, double *log_value);

/* The m most probable PAIRWISE DISTINCT full assignments of evidence set `batch` (the evidence jtp_set_evidence last gave it), in
 * descending value, by one upward max-product sweep whose message entries carry lists, and a decode per solution:
 *     states[s * n_vars + v] = state of variable v in solution s (a variable of no clique: 0)
 *     log_value[s] = log of the solution's unnormalised value prod_c psi_c(x)
 *     *n_found <= m = how many assignments of positive value there are; rows s >= *n_found are all -1, their log_value -inf, and
 *                     the call is still JTP_OK.
 * No propagate is needed, beliefs and messages are not touched.  1 <= m <= JTP_MBEST_MAX.
 * The sweep runs on the schedule of jtp_sample / jtp_map (by depth, then clique number; K_c = the variables clique c shares with its
 * parent clique, F_c the others in host axis order, R_c = prod card(F_c); children in ascending clique number), float64 throughout.
 * Upward, deepest first: every clique c and every assignment k of K_c gets a list raw_c[k][0..M) - non-increasing, zero past its
 * count, all zero where k contradicts the evidence - with a place (r, t) per element.  A child's message is read as m_d[k_d][j] =
 * ldexp(raw_d[k_d][j], -e_d), e_d = ilogb(max over k of raw_d[k][0]); element 0 of every list is jtp_map's raw, so the exponents
 * are jtp_map's.  Per entry (k, r) that agrees with the evidence, a fold over the children d_1, d_2, ...:
 *     E_0 = [(double)psi_c[k, r]]   (empty if that is 0)
 *     E_i = the M largest of the products E_{i-1}[a] * m_{d_i}[k_{d_i}][b] that are > 0, in descending value, equal values in ascending
 *           (a, b), lexicographically; every element remembers its (a, b)
 * (multiplication by a non-negative number is monotone, so only pairs with (a + 1) * (b + 1) <= M can be among them, and the order
 * among equals agrees with leaving the others out).  Per k, raw_c[k] = the M largest elements of the lists E_last of all such r, in
 * descending value, equal values in ascending (r, t), t the element's place in its list.  That is a total order: how r is cut into
 * lanes and segments does not matter.  Downward, per solution s: rank[root] = s; clique c reads (r, t) at (k from the digits written
 * above it, rank[c]), writes the digits of F_c from r, and follows element t of entry (k, r) back through the fold - the b of the
 * last step is the rank of the last child, its a the element of the step before, and so on; the device forms that one entry's
 * fold again, same operations in the same order, rather than keep a rank per child with every element.
 * log_value[s] = log(raw_root[0][s]) + ln 2 * (sum of e_c over the other cliques).
 * So: solution 0 of any call is jtp_map's result bit for bit, ties included; the first m' solutions of a call with m are the call with
 * m' < m (an element with a >= m' or b >= m' has m' elements before it) - the device runs lists of 1, 4 or 16 elements, the
 * smallest that holds m -; different ranks at one (clique, k) are different sub-assignments; an assignment whose scaled value
 * underflows to 0 is not listed; nothing depends on the plan's layout, compaction, root, launch flags, the "map_seg" knob or the
 * table type beyond the numbers held.
 * Works where jtp_map works: plans of one set, of n_batch sets and with JTP_SHARE_POTENTIALS, float32 and float64 tables, any layout;
 * the work area is that of one set, kept with the plan, grow-only.
 * JTP_EUNSUPPORTED: JTP_MULTISET plans, n_ranks > 1, plans in which a clique keeps no table (cover_*).  JTP_EINVAL: m < 1, m >
 * JTP_MBEST_MAX, a bad batch, null arguments.  The set FAILS as in jtp_map - an entry that agrees with its evidence is negative or
 * NaN, or a clique's largest first element is zero or not finite (evidence of probability zero) -: all m rows are -1, every log_value
 * -inf, *n_found = 0, the call returns JTP_EINVAL and the message says so. */
#define JTP_MBEST_MAX 16
int jtp_map_best(jtp_plan *plan, int32_t batch, int32_t m, int32_t *states, double *log_value, int32_t *n_found);

/* Marginal MAP: the most probable assignment of the query variables M = var_ids[0 .. n_query) with every other variable summed out,
 * m* = argmax_m sum_s prod_c psi_c(m, s), for every evidence set in [batch_begin, batch_end):
 *     states[(b - batch_begin) * n_query + i] = state of var_ids[i] in set b (an observed query variable: its observed state)
 *     log_value (NULL, or [batch_end - batch_begin]) = log max_m sum_s prod_c psi_c over what agrees with the set's evidence; less
 *                 jtp_get_log_z of the set it is log P(m* | evidence).
 * No propagate is needed, beliefs and messages are not touched; the evidence is what jtp_set_evidence last gave each set.
 * Max and sum do not commute, so the tree the plan was made from must be STRONG for the query: with K_c the variables clique c shares
 * with its parent clique and F_c its others, a clique whose F_c holds a variable of M has K_c inside M
 * (junctiontree_amd.construction.strong_junction_tree builds such a tree).  The call checks exactly that, before any device work.
 * The sweep runs over the tree as the description gave it, on the schedule of jtp_sample / jtp_map (by depth, then clique number;
 * F_c in host axis order; children in ascending clique number).  F_c is split into FM_c = F_c n M and FS_c = F_c \ M, each in host
 * axis order, Rm_c = prod card(FM_c), Rs_c = prod card(FS_c); rm and rs are the C-order indices over them.  Upward, deepest first,
 * float64 throughout, only entries that agree with the evidence looked at:
 *     U_c[k, rm] = sum over rs of ((double)psi_c[k, rm, rs] * m_1) * m_2 * ...     m_d = ldexp(raw_d[k_d], -e_d), e_d = ilogb(max raw_d)
 *     raw_c[k]   = max over rm of U_c[k, rm]          (0 where k contradicts the evidence)
 *     arg_c[k]   = the SMALLEST rm that attains it
 * The sum over rs is added in an order that is a function of Rs_c alone, jtp_joint's rule: min(64, Rs_c rounded up to a power of two)
 * lanes, lane l adds the contiguous block [l B, (l + 1) B) of rs, B = ceil(Rs_c / lanes), in ascending order, and a fixed tree of
 * shuffles adds the lanes; from Rs_c >= 2048 on, rs is first cut into min(4096, Rs_c / 1024) contiguous segments, each summed so, and
 * the segments' sums are added the same way (lane l those of segments l, l + 64, ...).  No floating-point atomics.  A maximum is exact,
 * so how rm is cut ("map_seg") does not matter: equal potentials and evidence give bit-equal states and log_value whatever the plan's
 * layout, compaction, launch flags, the chunking ("map_chunk") or any debug knob, and across repeated calls.
 * Downward: a clique with FM_c not empty reads arg_c[k] at the digits the cliques above wrote (K_c lies in M there) and writes the
 * digits of FM_c; a clique without FM_c writes nothing.  log_value = log(max raw_root) + ln 2 * (sum of e_c over the other cliques).
 * So: with M = all variables every Rs_c is 1 and the call IS jtp_map - the same kernels over the same records -, bit for bit: states,
 * ties and log_value.  With n_query = 0 it is the collect pass of sum-product, and log_value = log Z of the set.
 * All sets of a chunk go through the same launches; a chunk is as many sets as keep the raw and arg tables (12 bytes per assignment
 * of K_c) and the segment sums of the largest depth under 64 MiB.  The records of the last query are kept with the plan.
 * Works where jtp_map works: plans of one set, of n_batch sets and with JTP_SHARE_POTENTIALS, float32 and float64 tables, any layout.
 * JTP_EINVAL, before any device work: a query variable out of range, listed twice or in no clique; a bad batch range; null states
 * with n_query > 0; a tree that is not strong for the query ("clique c maximises variable x below variable y, which is summed and
 * shared with its parent clique p").  JTP_EUNSUPPORTED: JTP_MULTISET plans, n_ranks > 1, plans in which a clique keeps no table
 * (cover_*).  A set FAILS as in jtp_map - an entry that agrees with its evidence is negative or NaN, or a clique's largest raw entry
 * is zero or not finite (evidence of probability zero) -: its states are all -1, its log_value -inf; every set of the range is still
 * written, the call returns JTP_EINVAL and the message names the number of failed sets and the first. */
int jtp_marginal_map(jtp_plan *plan, int32_t batch_begin, int32_t batch_end, int32_t n_query, const int32_t *var_ids, int32_t *states,
                     double *log_value);

/* The joint of n_query distinct variables that need not share a clique, from the beliefs of the last propagate of evidence set
 * `batch`: host[] = the table over var_ids[0 .. n_query) in that axis order (doubles, C order).  Unnormalised in the sense of
 * jtp_get_marginal: it sums to Z, and on a JTP_SCALED plan it is the true table times 2^-E, E the exponent of the TOP clique below
 * (*log2_scale, if not NULL; what jtp_get_log2_scale reports for that clique; 0 without the flag).
 * The sweep runs over the tree as the description gave it, on the schedule of jtp_sample (by depth, then clique number; K_c = the
 * variables clique c shares with its parent clique, F_c the others in host axis order, R_c = prod card(F_c)).  The home of a query
 * variable is the shallowest clique that holds it; the top is the deepest clique whose subtree holds every home; only the cliques on
 * the paths from the homes up to the top are read.  With C_c = the query variables whose home lies in the subtree of c (in the
 * order of the query), Q_c those whose home is c, and r' running over the R'_c assignments of F_c without Q_c: upward, deepest
 * first, for every such clique but the top, every assignment k of K_c and x of C_c,
 *     sigma_c[k] = sum_r beta_c[k, r],   U_c[k, x] = sum_r' ((double)beta_c[k, x|Q_c, r'] * M_d1[.]) * M_d2[.] ...,
 *     M_c[k, x] = U_c[k, x] / sigma_c[k]   (0 where sigma_c[k] = 0)
 * - d1 < d2 < ... the children of c on those paths in ascending clique number, float64, left to right, each read at the digits of
 * K_d that (k, x, r') fix and at x restricted to C_d.  The top forms the same sum over all its variables outside the query, K_top
 * included, and does not divide.  A sum of n terms is added in an order that depends on n alone, so nothing depends on the plan's
 * layout, compaction, root or launch flags: equal beliefs give bit-equal joints.  The power of two a JTP_SCALED plan keeps per clique
 * cancels in U / sigma.  Observed variables need nothing special (the joint is zero off an observed state), evidence of probability
 * zero gives a joint of zeros and JTP_OK, and where every variable lies in one clique the result is that clique's marginal.
 * JTP_EINVAL: n_query < 1, a variable listed twice, out of range or of no clique, an evidence set never propagated.
 * JTP_EUNSUPPORTED, with the reason: JTP_MULTISET plans, n_ranks > 1, plans in which a clique keeps no table (cover_*); more than 16
 * variables; a result, or the sigma and M tables of a call together, beyond 64 MiB (the message names the clique that passes it and
 * the size of its M).  Where a belief entry read is negative or NaN, or a sum is not finite (tables that overflowed), the joint is
 * still written, the call returns JTP_EINVAL and the message names the number of such (clique, k) pairs and the first clique. */
int jtp_joint(jtp_plan *plan, int32_t batch, int32_t n_query, const int32_t *var_ids, double *host, int64_t *log2_scale);

/* Entropy of the posterior of every evidence set in [batch_begin, batch_end), and its cross-entropy against another propagated set
 * of the plan, in nats, from the beliefs the last propagates left: one streaming pass over ALL belief tables on the device.
 * On the schedule of jtp_sample (by depth, then clique number), for clique c: K_c = the variables c shares with its parent clique
 * (none at the root), F_c the others, R_c = prod card(F_c), n_c the entries of c; beta_c^b the belief of c in set b as the last
 * propagate left it, widened to float64 before anything else, entries that contradict the evidence already 0 in it;
 *     sigma_c[k] = sum_r beta_c[k, r],    S_c = sum_k sigma_c[k],
 * and for a set a and a reference set b (b = a: entropy)
 *     t_c(a, b) = sum_k [ sum_r beta_c^a[k, r] ln beta_c^b[k, r]  -  sigma_c^a[k] ln sigma_c^b[k] ].
 * Terms with beta_c^a = 0 (sigma_c^a[k] = 0) are left out - not multiplied: the logarithm is never taken of 0 on their account.
 *     h_c = -t_c(a, a) / S_c^a = H(F_c | K_c) under the posterior of a, >= 0;   x_c = -t_c(a, b) / S_c^a, the same conditional
 * cross-entropy against b, +inf (no error) where some beta^a > 0 meets beta^b = 0;   H(a) = sum_c h_c by the chain rule on the
 * tree - it depends neither on the root nor on the schedule, the single h_c do -;   X(a, b) = sum_c x_c;   KL(a || b) = X - H >= 0.
 * The power of two a JTP_SCALED plan keeps per node cancels inside t_c / S_c, for a and for b: no exponent is read.
 * entropy[batch_end - batch_begin]: H of each set.  ref_set and cross: both NULL, or ref_set[i] = the set b for set batch_begin + i
 * (any propagated set of the plan, inside the range or not) and cross[i] = X.  clique_entropy: NULL, or [sets x n_cliques], h_c by
 * clique number.  Beliefs and messages are not touched.  Works where jtp_sample works: one set or n_batch sets,
 * JTP_SHARE_POTENTIALS, float32 and float64 tables, every layout policy, compaction and launch flag, JTP_SCALED.
 * Every entry is read once (with a reference: once from each table).  The lanes of a wave take interleaved indices of F_c listed
 * in ascending DEVICE stride, so that they read consecutive elements; the order of a sum therefore depends on the stored layout:
 * plans of different layout agree to rounding - a few ulps times the length of the longest chain of additions, times max |ln beta| -
 * NOT bit for bit.  Two calls on the same plan and beliefs agree bit for bit: no floating-point atomics, no order that depends on
 * timing.  The cliques' terms are added in visit order.
 * JTP_EUNSUPPORTED, in jtp_sample's words: JTP_MULTISET plans, n_ranks > 1, plans in which a clique keeps no table (cover_*).
 * JTP_EINVAL before any device work: a bad range, entropy NULL, only one of ref_set and cross, a ref_set out of range, a set or
 * reference set never propagated.  A set FAILS where it or its reference holds a negative or NaN belief entry, or where an S_c of
 * it is zero or not finite (evidence of probability zero, overflow without JTP_SCALED): its outputs are NaN, every other set is
 * still written, the call returns JTP_EINVAL and the message names the number of failed sets and the first (set, clique). */
int jtp_entropy(jtp_plan *plan, int32_t batch_begin, int32_t batch_end, const int32_t *ref_set, double *entropy, double *cross,
                double *clique_entropy);

/* Expected counts: the weighted sum over evidence sets [batch_begin, batch_end) of the NORMALISED marginals of a request list
 * (requests as in jtp_get_marginals), formed and accumulated on the device:
 *     host[out_off[i] + h] = sum_b  weights[b - batch_begin] * m_bi[h] / S_bi ,   S_bi = sum_h m_bi[h]
 * m_bi = the marginal jtp_get_marginals(plan, b, ...) would return for request i.  weights NULL: all 1; they must be finite
 * (JTP_EINVAL before any device work), and a set of weight exactly 0 contributes nothing whatever its tables hold.
 * log_abs_z, z_sign (both NULL, or [batch_end - batch_begin] each): what jtp_get_log_z reports per set, weight 0 included.
 * Every request is divided by its own sum, so the power of two a JTP_SCALED plan keeps per node cancels.  Works wherever
 * jtp_get_marginals works on a plan of one rank (JTP_MULTISET, JTP_SHARE_POTENTIALS, n_batch, cover_*, JTP_SCALED);
 * n_ranks > 1: JTP_EUNSUPPORTED.  The sets are worked in chunks of as many as fit 64 MiB of partial copies (one host wait
 * per chunk, one copy back per call); S_bi is added in an order that depends on the request's entry count alone and a set is
 * added to the running sums after every set before it, so the result does not depend on the chunk size bit for bit.
 * A pair (b, i) with a nonzero weight whose S_bi is zero or not finite (evidence of probability zero, overflow on a plan without
 * JTP_SCALED) contributes nothing: every output is still written, the call returns JTP_EINVAL and the message names the number of
 * such pairs and the first (set, request).  Tables with negative entries are accepted as everywhere else, but the sums are
 * "counts" for non-negative models only. */
int jtp_accumulate_marginals(jtp_plan *plan, int32_t batch_begin, int32_t batch_end, const double *weights, int32_t n,
                             const int32_t *cliques, const int32_t *var_off, const int32_t *var_ids, const int64_t *out_off,
                             double *host, double *log_abs_z, int32_t *z_sign);

/* ---- instrumentation ------------------------------------------------------------------ */

/* Device timing of the next `keep` propagates with hipEvents on the plan's stream (ring; 0
 * switches it off).  per_launch = 0: three events per propagate (start, collect/distribute
 * boundary, end) - cheap enough to stay on in a timed benchmark region; per_launch = 1: an event
 * pair around every launch (about 4 us of idle GPU per event).  jtp_get_stats reports the mean
 * per propagate. */
int jtp_set_profiling(jtp_plan *plan, int32_t keep);
int jtp_set_profiling_granularity(jtp_plan *plan, int32_t per_launch);
/* Time only every `stride`-th propagate (the first one after this call included): an event costs 2-3 us of idle GPU, which a
 * benchmark of 0.6 ms propagates sees (1.3 % with every propagate timed).  Default 1. */
int jtp_set_profiling_stride(jtp_plan *plan, int32_t stride);
/* Device time of a whole REGION of work on the plan's (first) stream: jtp_region_begin records one event, jtp_region_end a
 * second one, waits for it and returns the milliseconds between them.  A benchmark brackets its K timed propagates with the
 * pair and divides by K: no event sits between the propagates, so the figure cannot exceed the wall-clock step. */
int jtp_region_begin(jtp_plan *plan);
int jtp_region_end(jtp_plan *plan, double *ms);
int jtp_get_stats(jtp_plan *plan, jtp_stats *stats);
/* Mean device time (ms) of each of the plan's launches, in schedule order; `n` = capacity of
 * `ms`.  Returns the number of launches (or a negative error).  Needs jtp_set_profiling. */
int jtp_get_launch_ms(jtp_plan *plan, double *ms, int32_t n);
/* Diagnostic: copy `n` doubles at offset `off` of evidence set `batch`'s message arena to the host. */
int jtp_debug_read_msg(jtp_plan *plan, int32_t batch, int64_t off, int64_t n, double *host);
/* Test hooks.  knob "flow_debug": JtFlow::dbg of the following propagates (8 = every dataflow wait times
 * out after 20 ms: exercises the fall-back to one launch per level); "flow": 0 = launch per level from now on;
 * "fail_alloc": see jtp_debug_live_bytes; "acc_chunk": evidence sets per chunk of jtp_accumulate_marginals (0: by size);
 * "map_chunk": the same of jtp_map and jtp_max_marginals; "map_seg": entries of r a wave of jtp_map and of jtp_max_marginals takes
 * (0: the default; the result does not depend on it). */
int jtp_debug_set(jtp_plan *plan, const char *knob, int64_t value);
/* Test hook: bytes of device memory and of pinned host memory the library holds right now, process-wide (every plan's buffers;
 * either pointer may be NULL).  With knob "fail_alloc" of jtp_debug_set (the N-th allocation of the plan from now on reports
 * out of memory on the host; 0 = off) and JTP_FAIL_ALLOC=N in the environment (the same for the allocations of
 * jtp_plan_create) it lets a test walk every allocation-failure path and see that nothing is left behind. */
int jtp_debug_live_bytes(int64_t *device_bytes, int64_t *pinned_bytes);
/* Name of kernel variant i as it appears in rocprofv3 traces, or NULL past the last one. */
const char *jtp_kernel_name(int32_t variant);

/* ---- multi-GPU: one process per GPU, RCCL point-to-point at subtree cuts --------------- */

/* Rank 0 creates a 128-byte RCCL unique id and hands it to the other ranks out of band. */
int jtp_comm_unique_id(void *id128);
/* Collective: every rank calls it once before creating plans with n_ranks > 1. */
int jtp_comm_init(int32_t rank, int32_t n_ranks, const void *id128, int32_t device);
int jtp_comm_destroy(void);
/* What the communicator itself reports: ncclCommCount, ncclCommUserRank, ncclCommCuDevice (-1 where the loaded library lacks
 * the entry point).  A multi-rank benchmark line quotes it, so that its reader sees RCCL saw N ranks. */
int jtp_comm_info(int32_t *n_ranks, int32_t *rank, int32_t *device);
/* Diagnostic: send `n` doubles from this rank to itself through the communicator (grouped
 * ncclSend + ncclRecv on a private stream) and verify them.  Exercises the RCCL binding on a
 * single GPU, where no second rank can exist. */
int jtp_comm_selftest(int32_t n);

/* ---- misc ----------------------------------------------------------------------------- */

int jtp_device_count(int32_t *count);
/* Free and total memory of a device (hipMemGetInfo): the Python layer budgets its plan cache with it. */
int jtp_device_memory(int32_t device, uint64_t *free_bytes, uint64_t *total_bytes);

/* Page-locked host memory for potentials and results: copies to and from it run at PCIe speed and
 * without an intermediate buffer (a pageable numpy array reads back at ~5 GB/s, a pinned one at
 * ~50).  Nothing in the reference corresponds (it has no device).  An array from here that was handed to
 * jtp_set_potential must stay alive and unmodified until jtp_sync (see the lifetime rule there). */
int jtp_host_alloc(void **ptr, size_t bytes);
int jtp_host_free(void *ptr);
const char *jtp_last_error(void);
const char *jtp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* JTPROP_H */
