// CDNA4 (gfx950) kernels of the junction-tree message-passing hot path: their face.
//
// This file declares every message-passing kernel and lists the explicit instantiations; it holds no bodies.  The engine
// (jtp_propagate.hip) includes it to take the kernels' addresses and depends on nothing else of them.  The bodies live in units by
// concern, and every jtp_inst_<family>_<type>.hip includes the unit of its family alone:
//
//   jtp_k_common.h   constants of the row ring, LDS-DMA, shuffles, time stamps, the marker protocol, flow_ctl and the ticket
//   jtp_k_pass.h     jt_pass: the one body of the table-keeping passes, both directions            <- common
//   jtp_k_reduce.h   jt_reduce: the sum of a message's partial copies                               <- common
//   jtp_k_lean.h     jt_unit_lean, its dispatchers and jt_lean_block: unit tasks without the interpretation   <- common
//   jtp_k_unit.h     jt_unit_collect / _distribute / _single: unit tasks to the generic or the lean pass      <- pass, lean
//   jtp_k_level.h    family level: one launch per tree level, and the read-out task lists           <- reduce, unit
//   jtp_k_flow.h     families flow, both, bothm: one launch per phase or per propagate (dataflow)    <- reduce, unit
//   jtp_k_mix.h      families mix, mixc: the same launches for mixed-radix rows                     <- reduce, unit
//   jtp_k_multi.h    family multi: jt_mpass and jt_multi_flow, eight evidence sets per table read    <- common, reduce
//   jtp_k_shape.h    family shape: one kernel per clique shape (JTP_SPLIT_VARIANTS)                  <- pass
//
// (build.py reads these edges from the #include lines: an edit to jt_mpass recompiles the two multi units and nothing else.)
//
// Launch structure: by default ONE launch per phase (jt_collect_flow / jt_distribute_flow) or per propagate (jt_propagate_flow) over
// the block list of all tree levels; a workgroup that finds a message entry still marked unwritten waits for it (FLOW = true in
// jt_pass).  The same body runs once per tree level in jt_*_level and once per level and clique shape in jt_collect<> /
// jt_distribute<> (timing aids, and the fallback).
#pragma once
#include <hip/hip_runtime.h>

#include "jtp_internal.h"

#define JT_KARGS(T) const JtTask *, const JtBlock *, const int *, const T *, T *, double *, JtFlow

// family level (jtp_k_level.h)
template <typename T> __global__ void jt_reduce_level(JT_KARGS(T));
template <typename T> __global__ void jt_collect_level(JT_KARGS(T));
template <typename T> __global__ void jt_distribute_level(JT_KARGS(T));
template <typename T> __global__ void jt_single(JT_KARGS(T));
template <typename T> __global__ void jt_lean_single(JT_KARGS(T));
template <typename T> __global__ void jt_marginals(JT_KARGS(T));
// families flow, both and bothm (jtp_k_flow.h)
template <typename T> __global__ void jt_collect_flow(JT_KARGS(T));
template <typename T> __global__ void jt_collect_flow_keep(JT_KARGS(T));
template <typename T> __global__ void jt_propagate_flow(JT_KARGS(T));
template <typename T> __global__ void jt_propagate_flow_marg(JT_KARGS(T));
template <typename T> __global__ void jt_distribute_flow(JT_KARGS(T));
template <typename T> __global__ void jt_distribute_flow_chain(JT_KARGS(T));
// family multi (jtp_k_multi.h)
template <typename T> __global__ void jt_multi_flow(JT_KARGS(T));
// families mix (VG = false) and mixc (VG = true) (jtp_k_mix.h)
template <typename T, bool VG = false> __global__ void jt_collect_level_mix(JT_KARGS(T));
template <typename T, bool VG = false> __global__ void jt_distribute_level_mix(JT_KARGS(T));
template <typename T, bool VG = false> __global__ void jt_single_mix(JT_KARGS(T));
template <typename T, bool VG = false> __global__ void jt_collect_flow_mix(JT_KARGS(T));
template <typename T, bool VG = false> __global__ void jt_distribute_flow_mix(JT_KARGS(T));
// family shape (jtp_k_shape.h)
template <typename T, int NCH> __global__ void jt_collect(JT_KARGS(T));
template <typename T, int HASP, int NCH> __global__ void jt_distribute(JT_KARGS(T));

// ------------------------------------------------------------------------------------------
// Explicit instantiation lists.  The message-passing kernels are compiled in translation units of their own, in parallel
// (jtp_inst_*.hip: one family and storage type each; build.py), every other translation unit sees them as `extern template`:
// one translation unit with everything took 3.5 minutes to compile.  X = `extern` or nothing.
#define JT_INST_FLOW(X, T)                                                   \
    X template __global__ void jt_collect_flow<T>(JT_KARGS(T));              \
    X template __global__ void jt_collect_flow_keep<T>(JT_KARGS(T));         \
    X template __global__ void jt_distribute_flow<T>(JT_KARGS(T));           \
    X template __global__ void jt_distribute_flow_chain<T>(JT_KARGS(T));
#define JT_INST_LEVEL(X, T)                                                  \
    X template __global__ void jt_collect_level<T>(JT_KARGS(T));             \
    X template __global__ void jt_distribute_level<T>(JT_KARGS(T));          \
    X template __global__ void jt_reduce_level<T>(JT_KARGS(T));              \
    X template __global__ void jt_single<T>(JT_KARGS(T));                    \
    X template __global__ void jt_lean_single<T>(JT_KARGS(T));               \
    X template __global__ void jt_marginals<T>(JT_KARGS(T));
#define JT_INST_SHAPE(X, T)                                                  \
    X template __global__ void jt_collect<T, 0>(JT_KARGS(T));                \
    X template __global__ void jt_collect<T, 1>(JT_KARGS(T));                \
    X template __global__ void jt_collect<T, 2>(JT_KARGS(T));                \
    X template __global__ void jt_collect<T, 3>(JT_KARGS(T));                \
    X template __global__ void jt_distribute<T, 0, 0>(JT_KARGS(T));          \
    X template __global__ void jt_distribute<T, 0, 1>(JT_KARGS(T));          \
    X template __global__ void jt_distribute<T, 0, 2>(JT_KARGS(T));          \
    X template __global__ void jt_distribute<T, 0, 3>(JT_KARGS(T));          \
    X template __global__ void jt_distribute<T, 1, 0>(JT_KARGS(T));          \
    X template __global__ void jt_distribute<T, 1, 1>(JT_KARGS(T));          \
    X template __global__ void jt_distribute<T, 1, 2>(JT_KARGS(T));          \
    X template __global__ void jt_distribute<T, 1, 3>(JT_KARGS(T));
#define JT_INST_MULTI(X, T) X template __global__ void jt_multi_flow<T>(JT_KARGS(T));
// (the two kernels of a propagate in one launch are the largest of all - together 20 minutes of one compiler - so each has a
//  translation unit of its own: jtp_inst_both_*.hip and jtp_inst_bothm_*.hip)
#define JT_INST_BOTH(X, T) JT_INST_PROPAGATE(X, T) JT_INST_PROPAGATE_MARG(X, T)
#define JT_INST_PROPAGATE(X, T) X template __global__ void jt_propagate_flow<T>(JT_KARGS(T));
#define JT_INST_PROPAGATE_MARG(X, T) X template __global__ void jt_propagate_flow_marg<T>(JT_KARGS(T));
#define JT_INST_MIX_V(X, T, V)                                                  \
    X template __global__ void jt_collect_level_mix<T, V>(JT_KARGS(T));         \
    X template __global__ void jt_distribute_level_mix<T, V>(JT_KARGS(T));      \
    X template __global__ void jt_single_mix<T, V>(JT_KARGS(T));                \
    X template __global__ void jt_collect_flow_mix<T, V>(JT_KARGS(T));          \
    X template __global__ void jt_distribute_flow_mix<T, V>(JT_KARGS(T));
#define JT_INST_MIX(X, T) JT_INST_MIX_V(X, T, false)
#define JT_INST_MIXC(X, T) JT_INST_MIX_V(X, T, true)
#ifndef JT_INST_TU
JT_INST_FLOW(extern, float)
JT_INST_FLOW(extern, double)
JT_INST_LEVEL(extern, float)
JT_INST_LEVEL(extern, double)
JT_INST_SHAPE(extern, float)
JT_INST_SHAPE(extern, double)
JT_INST_MULTI(extern, float)
JT_INST_MULTI(extern, double)
JT_INST_BOTH(extern, float)
JT_INST_BOTH(extern, double)
JT_INST_MIX(extern, float)
JT_INST_MIX(extern, double)
JT_INST_MIXC(extern, float)
JT_INST_MIXC(extern, double)
#endif
