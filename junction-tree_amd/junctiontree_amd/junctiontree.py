"""User interface of the junction-tree library, MI355X build.

Same public names and data model as the reference's `junctiontree/junctiontree.py`:
`create_junction_tree(factors, sizes)` (:12-16) returns a `JunctionTree` whose
`propagate(values)` (:297-331) turns factor values into consistent, unnormalised factor
marginals.  Structure classes are plain Python; all numeric work of `propagate` after the
factor product runs on the GPU through `engine.Plan`:

    values --H2D (factor tables only)--> clique potentials formed on the device (evaluate,
    junctiontree.py:203-226) --> collect + distribute (computation.py:37-246 in one plan) -->
    per-factor marginals on the device (junctiontree.py:264-274) --D2H--> list shaped like `values`.
"""

from dataclasses import dataclass, field
from typing import Any

import numpy as np

from . import construction as cons

__all__ = ["create_junction_tree", "argfind1", "take", "is_subset", "einsum",
           "FactorGraph", "CliqueGraph", "JunctionTree"]


def create_junction_tree(factors, sizes, order=None):
    """Create a junction tree for a factor graph (reference: `junctiontree.py:12-16`).  `order` (not in the reference):
    an elimination order for the triangulation instead of greedy min-fill (`construction.triangulate`)."""
    assert all(type(f) == list for f in factors), "Provided factor is not a list"
    return FactorGraph(factors=factors, sizes=sizes).triangulate(order=order).create_junction_tree()


def argfind1(xs, cond):
    """Index of the first element of xs satisfying cond (`junctiontree.py:19-21`)."""
    for i, x in enumerate(xs):
        if cond(x):
            return i
    raise StopIteration


def take(xs, inds):
    """Pick several list elements (`junctiontree.py:24-26`)."""
    return [xs[i] for i in inds]


def is_subset(a, b):
    """Whether every element of a is in b (`junctiontree.py:29-31`)."""
    return set(a) <= set(b)


def einsum(xs, xs_keys, y_keys):
    """Product of arrays onto `y_keys` with arbitrary labels; labels that appear only in
    the output become length-1 axes (reference helper `junctiontree.py:34-80`).  Host-side
    (numpy): it builds clique potentials from factor tables, outside the message-passing
    path."""
    xs = [np.asarray(x) for x in xs]
    xs_keys = [list(k) for k in xs_keys]
    have = set(k for keys in xs_keys for k in keys)
    fresh = [k for k in y_keys if k not in have]
    if fresh:
        xs[0] = xs[0].reshape((1,) * len(fresh) + xs[0].shape)
        xs_keys[0] = fresh + xs_keys[0]
    number = {}
    for keys in xs_keys + [list(y_keys)]:
        for k in keys:
            number.setdefault(k, len(number))
    call = []
    for x, keys in zip(xs, xs_keys):
        call += [x, [number[k] for k in keys]]
    call.append([number[k] for k in y_keys])
    return np.einsum(*call)


def _normalised(tables):
    """Every table divided by its own sum (a table that sums to zero - evidence of probability zero - stays as it is)."""
    out = []
    for t in tables:
        total = t.sum()
        out.append(t / total if total != 0 else t)
    return out


def _stage_changed_cliques(plan, ct, xs, changed=None):
    """`evaluate` on the device for the cliques whose member factors differ from what `plan` holds: one call into the
    library for all of them (`engine.Plan.stage_factors`).  Returns the number of cliques formed (`plan.staged_cliques`
    keeps the count of the last call for tests and tools).  What is staged = which factors, over which variables in which
    axis order, with which values: two JunctionTree objects whose junction trees coincide share one cached plan
    (`engine.plan_for` keys on the tree, not on the factors), and the same bytes under a transposed label list are
    another table - `stage_factors` compares all of that, unless the caller names the changed factors (`changed`)."""
    return plan.stage_factors(ct.factor_graph.factors, ct.factor_to_maxclique, xs, changed=changed)


@dataclass(frozen=True)
class FactorGraph:
    """Factors (lists of variables) and the size of every variable (`junctiontree.py:83-117`)."""

    factors: Any
    sizes: Any

    def triangulate(self, order=None):
        """Triangulate and collect the maximal cliques (`junctiontree.py:102-117`)."""
        maxcliques, factor_to_maxclique = cons.triangulate(self.factors, self.sizes, order=order)
        return CliqueGraph(maxcliques=maxcliques, factor_to_maxclique=factor_to_maxclique,
                           factor_graph=self)


@dataclass
class CliqueGraph:
    """Maximal cliques of a triangulated factor graph (`junctiontree.py:120-274`)."""

    maxcliques: Any
    factor_to_maxclique: Any
    factor_graph: Any

    def create_junction_tree(self):
        """`junctiontree.py:138-200`: node list = maxcliques ++ separators, tree of indices."""
        tree, separators = cons.construct_junction_tree(self.maxcliques, self.factor_graph.sizes)
        return JunctionTree(tree=tree, separators=separators, clique_tree=self)

    def _members(self):
        members = [[] for _ in self.maxcliques]
        for fi, mc in enumerate(self.factor_to_maxclique):
            members[mc].append(fi)
        return members

    def evaluate(self, xs):
        """Clique values from factor values (`junctiontree.py:203-226`): the product of the
        factors assigned to each clique in the clique's axis order; variables no assigned
        factor covers stay length-1 axes."""
        out = []
        for clique, members in zip(self.maxcliques, self._members()):
            if not members:
                out.append(np.ones((1,) * len(clique)))
                continue
            out.append(einsum(take(xs, members), take(self.factor_graph.factors, members), clique))
        return out

    def marginalize(self, ys):
        """Factor results from clique results (`junctiontree.py:229-274`) for arrays already
        on the host: sum the clique axes that are not in the factor."""
        return [einsum([ys[mc]], [self.maxcliques[mc]], list(fvars))
                for fvars, mc in zip(self.factor_graph.factors, self.factor_to_maxclique)]


@dataclass(frozen=True)
class JunctionTree:
    """Junction tree of a factor graph (`junctiontree.py:277-331`).

    `tree` = [clique, (separator, subtree), ...] over the node list
    `clique_tree.maxcliques + separators`."""

    tree: Any
    separators: Any
    clique_tree: Any
    _opts: dict = field(default_factory=dict, compare=False, repr=False)
    _memo: dict = field(default_factory=dict, compare=False, repr=False)

    # what a tree remembers between calls (a weak reference to its device plan, derived tables) is not part of its value:
    # a tree pickles and copies like the reference's, before and after it has been used
    def __getstate__(self):
        state = dict(self.__dict__)
        state["_memo"] = {}
        return state

    def __setstate__(self, state):
        for k, v in state.items():
            object.__setattr__(self, k, v)

    def cover(self, trusted=False):
        """Per clique, the variables its potential depends on: the union of the variables of the factors assigned to it
        (`junctiontree.py:203-226` - evaluate leaves every other variable of the clique a length-1 axis, `:52-61`).  The device
        plan keeps no full-size table for a clique that is mostly such axes (`engine.Plan(cover=...)`).  `trusted`: the caller
        vouches that the factor lists are what they were at the last call (`propagate(xs, changed=...)`): the remembered
        cover is returned without looking at them."""
        from .engine import _same_lists as engine_same_lists
        ct = self.clique_tree
        hit = self._memo.get("cover")
        if trusted and hit is not None:
            return hit[1]
        # (compared by value against list copies - list.__eq__ runs in C; hit[0] is a version number `plan` keys on)
        if hit is not None and hit[3] == list(ct.factor_to_maxclique) and engine_same_lists(hit[2], ct.factor_graph.factors):
            return hit[1]
        cover = [[] for _ in ct.maxcliques]
        scalar = [False] * len(ct.maxcliques)
        for fvars, mc in zip(ct.factor_graph.factors, ct.factor_to_maxclique):
            scalar[mc] = scalar[mc] or len(fvars) == 0
            for v in fvars:
                if v not in cover[mc]:
                    cover[mc].append(v)
        for mc, clique in enumerate(ct.maxcliques):
            if scalar[mc]:                                   # (a factor without variables is a value no axis carries: the clique keeps its table)
                cover[mc] = list(clique)
        self._memo["cover"] = ((hit[0] + 1) if hit is not None else 0, cover, [list(f) for f in ct.factor_graph.factors], list(ct.factor_to_maxclique))
        return cover

    # results of the last `propagate(..., normalize=True)` / `propagate_evidence_sets(..., normalize=True)`: log|Z| and the sign of Z
    # (the reference allows signed values), one log|Z_e| per evidence set
    @property
    def log_z(self):
        return self._memo.get("log_z")

    @property
    def z_sign(self):
        return self._memo.get("z_sign")

    @property
    def log_z_sets(self):
        return self._memo.get("log_z_sets")

    def plan(self, dtype="f64", trusted=False, fold=True, scaled=False):
        """The device plan for the current variable sizes (sizes are read at call time, as
        `junctiontree.py:311` does: the reference's tests condition on evidence by setting
        a size to 1, `tests/test_junctiontree.py:393-411`)."""
        import weakref
        from . import engine

        # the plan cache's key names the whole structure (1-2 ms to build for a thousand cliques): a tree remembers the key
        # and a weak reference to the plan it was last given for (dtype, the sizes as they are NOW, its options, and the
        # factor structure its cover was computed from - by value: a recomputed cover may reuse the old list's id)
        sizes = self.clique_tree.factor_graph.sizes
        # (`scaled`: the overflow-safe plan of `propagate(xs, normalize=True)` - an entry of its own, so that what the default call
        #  trusts about "plan" is never said of another plan)
        memo = ("plan" if fold else "plan_nofold") + ("_scaled" if scaled else "")
        hit = self._memo.get(memo)
        if trusted and hit is not None and hit[0][0] == dtype:      # (`propagate(xs, changed=...)`: sizes, options and factors are vouched for)
            plan = engine.cached_plan(hit[1], hit[2]())
            if plan is not None:
                return plan
        cover = self.cover(trusted=trusted)
        mark = (dtype, tuple(sizes.items()), tuple(sorted(self._opts.items())), self._memo["cover"][0])
        if hit is not None and hit[0] == mark:
            plan = engine.cached_plan(hit[1], hit[2]())
            if plan is not None:
                return plan
        node_vars = [list(c) for c in self.clique_tree.maxcliques] + [list(s) for s in self.separators]
        # (`fold`: propagate returns factor marginals only, junctiontree.py:327-331 - the plan is told which, so that those of cliques
        #  without a table are formed inside the propagate's launch; fold=False: the plan `compute_beliefs` would make of this tree)
        ct = self.clique_tree
        extra = {"fold": (tuple(ct.factor_to_maxclique), tuple(map(tuple, ct.factor_graph.factors)))} if fold else {}
        if scaled:
            extra["scaled"] = True
        plan, key = engine.plan_for(self.tree, node_vars, sizes, dtype, return_key=True, cover=cover, **extra, **self._opts)
        self._memo[memo] = (mark, key, weakref.ref(plan))
        return plan

    def propagate(self, xs, changed=None, normalize=False):
        """Belief propagation: factor values in, unnormalised factor marginals out (same
        list length and array shapes as `xs`; float64).

        `normalize` (not in the reference, which has no overflow control): the propagate runs on an overflow-safe plan - every
        message is divided by a power of two as it is produced, `engine.Plan(scaled=True)` - and every returned marginal is divided
        by its own sum; `tree.log_z` is then log|Z| and `tree.z_sign` the sign of Z, finite where Z itself is beyond float64.

        `changed` (not in the reference; it answers the FIXME at `junctiontree.py:206-214`): the indices of the factors whose
        tables differ from the previous call on this tree, or "all".  By default every table is compared with what the device
        holds (one vectorised pass over all of them, so that arrays updated in place are seen); a caller that knows what it
        changed skips that - and vouches that the factor structure and every other table are what they were."""
        ct = self.clique_tree
        trusted = changed is not None and ("plan_scaled" if normalize else "plan") in self._memo
        if trusted and "all_f32" in self._memo:          # (the caller vouches for the structure - shapes and dtypes with it)
            all_f32 = self._memo["all_f32"]
        else:
            all_f32 = self._memo["all_f32"] = all(type(x) is np.ndarray and x.dtype == np.float32 for x in xs)
        plan = self.plan("f32" if all_f32 else "f64", trusted=trusted, scaled=normalize)
        # evaluate (junctiontree.py:203-226) on the device: only factor tables cross PCIe, and only those of
        # cliques whose factors changed since this plan last saw them (the reference recomputes every clique on
        # every call and says so in a FIXME, junctiontree.py:206-214)
        _stage_changed_cliques(plan, ct, xs, changed=changed)
        # (no wait here: `jtp_get_marginals` waits.  After a dataflow propagate it first waits for the stream and looks at the abort flag
        #  (settle), then enqueues the marginal kernels; only behind per-level launches are they enqueued while the propagate runs)
        plan.propagate(sync=False)
        # marginalize (junctiontree.py:229-274) on the device: one launch for all factors, the factors of one clique
        # sharing the passes over its belief table
        out = plan.factor_marginals(ct.factor_graph.factors, ct.factor_to_maxclique, trusted=trusted)
        if normalize:
            self._memo["z_sign"], self._memo["log_z"] = plan.log_z()
            out = _normalised(out)
        return out

    def sample(self, values, n, seed=0, evidence=None, normalize=False):
        """`n` joint samples from the distribution the factor values define (not in the reference, which stops at marginals):
        {variable: int32 array of length n}, sample i being entry i of every array (views of one array).  `evidence`:
        {variable: observed state} - the samples are then draws from the posterior, with the observed variables in their
        observed states.  `normalize`: the propagate behind the samples runs on an overflow-safe plan (`engine.Plan(scaled=True)`),
        for models whose Z lies beyond float64.  Counter based: the same `seed` gives the same samples, and the first samples of a
        longer call are those of a shorter one (`synthetic.sample_uniform`).  The factor values must give non-negative beliefs: a draw
        that meets a negative belief entry raises `_capi.JtpError` (its `states`: -1 for what could not be drawn), as one of probability zero does.

        The draw is one root-to-leaves sweep over the clique beliefs on the device (`engine.Plan.sample`), so every clique table is
        materialised: the plan is made without `cover`, unlike `propagate`'s.  On lattice-like models, whose cliques are mostly
        variables no factor of theirs covers, that is many times the memory - 9 GiB for the 6 x 167 lattice of cardinality 8
        (BASELINE configs[2]) against the few MiB `propagate` needs."""
        import weakref
        from . import engine

        ct = self.clique_tree
        sizes = ct.factor_graph.sizes
        all_f32 = all(type(x) is np.ndarray and x.dtype == np.float32 for x in values)
        dtype = "f32" if all_f32 else "f64"
        # (an entry of its own: what `propagate(xs, changed=...)` trusts about "plan" is never said of this plan)
        memo = "plan_sample" + ("_scaled" if normalize else "")
        mark = (dtype, tuple(sizes.items()), tuple(sorted(self._opts.items())))
        hit = self._memo.get(memo)
        plan = engine.cached_plan(hit[1], hit[2]()) if hit is not None and hit[0] == mark else None
        if plan is None:
            node_vars = [list(c) for c in ct.maxcliques] + [list(s) for s in self.separators]
            extra = {"scaled": True} if normalize else {}
            plan, key = engine.plan_for(self.tree, node_vars, sizes, dtype, return_key=True, **extra, **self._opts)
            self._memo[memo] = (mark, key, weakref.ref(plan))
        _stage_changed_cliques(plan, ct, values)
        plan.set_evidence(dict(evidence) if evidence else {})
        try:
            plan.propagate(sync=False)
            states = plan.sample(n, seed=seed)
        finally:
            if evidence:                                     # (the plan is the cache's: whoever is handed it next finds no evidence set)
                plan.set_evidence({})
        out = {lab: states[:, j] for j, lab in enumerate(plan.var_labels)}
        for lab in plan._trivial:                            # (one-state variables the plan keeps on the host)
            out[lab] = np.zeros(int(n), dtype=np.int32)
        for lab in sizes:                                    # (variables of no clique cannot occur: every variable is in a factor)
            out.setdefault(lab, np.zeros(int(n), dtype=np.int32))
        return out

    def joint(self, values, variables, evidence=None, normalize=False):
        """The joint distribution of `variables` - a list of distinct variables that need not share a factor or a clique - under the
        distribution the factor values define (not in the reference, which stops at the marginals of its factors): a float64 array
        with one axis per variable, in the order given.  `evidence`: {variable: observed state} - the table is then that of the
        posterior, zero off the observed state of an observed variable.  Without `normalize` the table is unnormalised, as the
        marginals of `propagate` are: it sums to Z (times the probability of the evidence).  `normalize`: the propagate behind it
        runs on an overflow-safe plan (`engine.Plan(scaled=True)`) and the table is divided by its sum - a probability table, also
        where Z lies beyond float64; evidence of probability zero then raises `_capi.JtpError`.

        One propagate, then one upward sweep on the device over the cliques between the variables (`engine.Plan.joint`), where
        clamping one variable to each of its states in turn costs a propagate per state.  A negative belief entry in one of those
        cliques (signed factor values) raises `_capi.JtpError` naming the clique; cliques the sweep does not read may hold what they like.

        The sweep reads the clique beliefs, so every clique table is materialised: the plan is made without `cover`, unlike
        `propagate`'s.  On lattice-like models, whose cliques are mostly variables no factor of theirs covers, that is many times the
        memory - 9 GiB for the 6 x 167 lattice of cardinality 8 (BASELINE configs[2]) against the few MiB `propagate` needs."""
        import weakref
        from . import engine
        from ._capi import JtpError

        ct = self.clique_tree
        sizes = ct.factor_graph.sizes
        variables = list(variables)
        for lab in variables:
            if lab not in sizes:
                raise ValueError("variable %r is not a variable of the model" % (lab,))
        if len(set(variables)) != len(variables):
            raise ValueError("a variable is listed twice: %r" % (variables,))
        if not variables:
            raise ValueError("at least one variable")
        all_f32 = all(type(x) is np.ndarray and x.dtype == np.float32 for x in values)
        dtype = "f32" if all_f32 else "f64"
        # (an entry of its own, as `sample` keeps: what `propagate(xs, changed=...)` trusts about "plan" is never said of this plan)
        memo = "plan_joint" + ("_scaled" if normalize else "")
        mark = (dtype, tuple(sizes.items()), tuple(sorted(self._opts.items())))
        hit = self._memo.get(memo)
        plan = engine.cached_plan(hit[1], hit[2]()) if hit is not None and hit[0] == mark else None
        if plan is None:
            node_vars = [list(c) for c in ct.maxcliques] + [list(s) for s in self.separators]
            extra = {"scaled": True} if normalize else {}
            plan, key = engine.plan_for(self.tree, node_vars, sizes, dtype, return_key=True, **extra, **self._opts)
            self._memo[memo] = (mark, key, weakref.ref(plan))
        _stage_changed_cliques(plan, ct, values)
        plan.set_evidence(dict(evidence) if evidence else {})
        try:
            plan.propagate(sync=False)
            table, _ = plan.joint(variables)
        finally:
            if evidence:                                     # (the plan is the cache's: whoever is handed it next finds no evidence set)
                plan.set_evidence({})
        if normalize:
            total = table.sum()
            if not total > 0.0:
                raise JtpError("joint: the table sums to %r - evidence of probability zero has no posterior to normalise" % (float(total),))
            table = table / total
        return table

    def _table_plan(self, memo, dtype, normalize, **extra):
        """The cached plan with every clique table materialised (no `cover`) that the information measures run on: an entry of
        its own per `memo`, as `sample` and `joint` keep - what `propagate(xs, changed=...)` trusts about "plan" is never said of it."""
        import weakref
        from . import engine

        ct = self.clique_tree
        sizes = ct.factor_graph.sizes
        memo += "_scaled" if normalize else ""
        mark = (dtype, tuple(sorted(extra.items())), tuple(sizes.items()), tuple(sorted(self._opts.items())))
        hit = self._memo.get(memo)
        plan = engine.cached_plan(hit[1], hit[2]()) if hit is not None and hit[0] == mark else None
        if plan is None:
            node_vars = [list(c) for c in ct.maxcliques] + [list(s) for s in self.separators]
            if normalize:
                extra = dict(extra, scaled=True)
            plan, key = engine.plan_for(self.tree, node_vars, sizes, dtype, return_key=True, **extra, **self._opts)
            self._memo[memo] = (mark, key, weakref.ref(plan))
        return plan

    def entropy(self, values, evidence=None, normalize=False):
        """The entropy, in nats, of the distribution the factor values define - of the posterior given `evidence` ({variable:
        observed state}) - as a float (not in the reference, which stops at marginals): H = sum over the cliques of the conditional
        entropy of a clique's own variables given those it shares with its parent, one streaming pass over the clique beliefs on
        the device (`engine.Plan.entropy`).  `normalize`: the propagate behind it runs on an overflow-safe plan
        (`engine.Plan(scaled=True)`), for models whose Z lies beyond float64.  Evidence of probability zero, and factor values that
        give a negative belief entry, raise `_capi.JtpError`.  Every clique table is materialised, as for `sample` and `joint`."""
        return float(self.entropy_evidence_sets(values, [dict(evidence) if evidence else {}], normalize=normalize)[0])

    def entropy_evidence_sets(self, values, evidence_sets, normalize=False):
        """`entropy` for several evidence sets over the same factor values: a float64 array, one copy of the clique tables and
        one call on the device for all sets.  A set whose evidence has probability zero raises `_capi.JtpError`, carrying
        `entropy` (NaN for that set, the others written)."""
        n_sets = len(evidence_sets)
        if n_sets == 0:
            return np.zeros(0)
        ct = self.clique_tree
        all_f32 = all(type(x) is np.ndarray and x.dtype == np.float32 for x in values)
        plan = self._table_plan("plan_entropy", "f32" if all_f32 else "f64", normalize, n_batch=n_sets, share_potentials=True)
        _stage_changed_cliques(plan, ct, values)
        try:
            for b, observed in enumerate(evidence_sets):
                plan.set_evidence(dict(observed) if observed else {}, batch=b)
            plan.propagate(sync=False)
            return plan.entropy(0, n_sets)
        finally:
            for b, observed in enumerate(evidence_sets):     # (the plan is the cache's: whoever is handed it next finds no evidence set)
                if observed:
                    plan.set_evidence({}, batch=b)

    def kl_divergence(self, values_p, values_q, evidence=None, normalize=False):
        """KL(P || Q) in nats between the distributions two lists of factor values define over this tree's factors - between their
        posteriors given the same `evidence` -: a float, `inf` where Q gives probability zero to something P does not.  Both value
        lists are staged on one plan of two evidence sets, propagated, and one pass over both sets' clique beliefs forms the entropy
        of P and its cross-entropy against Q (`engine.Plan.entropy(ref=...)`); the difference is returned, no less than 0.0."""
        ct = self.clique_tree
        all_f32 = all(type(x) is np.ndarray and x.dtype == np.float32 for vs in (values_p, values_q) for x in vs)
        plan = self._table_plan("plan_kl", "f32" if all_f32 else "f64", normalize, n_batch=2)
        factors = ct.factor_graph.factors
        try:
            for b, vs in enumerate((values_p, values_q)):
                for c in range(len(ct.maxcliques)):
                    members = [f for f, mc in enumerate(ct.factor_to_maxclique) if mc == c]
                    plan.set_potential_product(c, [vs[f] for f in members], [list(factors[f]) for f in members], batch=b)
                plan.set_evidence(dict(evidence) if evidence else {}, batch=b)
            plan.propagate(sync=False)
            h, x = plan.entropy(0, 1, ref=1)
        finally:
            if evidence:
                for b in range(2):
                    plan.set_evidence({}, batch=b)
        return float("inf") if np.isinf(x[0]) else max(float(x[0] - h[0]), 0.0)

    def map(self, values, evidence=None):
        """The most probable joint assignment under the distribution the factor values define (not in the reference, which stops
        at marginals): ({variable: state}, log_value), log_value = log of the product of the factor values at that assignment -
        less log Z (`propagate(values, normalize=True)`, then `tree.log_z`) it is the assignment's log probability.  `evidence`:
        {variable: observed state} - the most probable explanation of that observation.  See `map_evidence_sets`."""
        states, value = self.map_evidence_sets(values, [dict(evidence) if evidence else {}])
        return {lab: int(col[0]) for lab, col in states.items()}, float(value[0])

    def map_evidence_sets(self, values, evidence_sets):
        """`map` for several evidence sets over the same factor values: ({variable: int32 array of length n_sets}, float64 array of
        the sets' log values), all sets through the same launches of one max-product sweep on the device (`engine.Plan.map`) over
        one copy of the clique tables.  Models whose Z lies beyond float64 need nothing special: the sweep rescales its messages
        by powers of two and reports a logarithm.  A set whose evidence has probability zero raises `_capi.JtpError`, carrying
        `states` (-1 for that set) and `log_value` (-inf) as `engine.Plan.map` does.

        The sweep reads every clique table, so every clique table is materialised: the plan is made without `cover`, unlike
        `propagate`'s.  On lattice-like models, whose cliques are mostly variables no factor of theirs covers, that is many times the
        memory - 9 GiB for the 6 x 167 lattice of cardinality 8 (BASELINE configs[2]) against the few MiB `propagate` needs."""
        sizes = self.clique_tree.factor_graph.sizes
        n_sets = len(evidence_sets)
        if n_sets == 0:
            return {lab: np.zeros(0, dtype=np.int32) for lab in sizes}, np.zeros(0)

        def sweep(plan):
            try:
                states, value = plan.map(0, n_sets)
            except Exception as exc:
                if hasattr(exc, "states"):
                    exc.states = self._map_columns(plan, exc.states, sizes)
                raise
            return self._map_columns(plan, states, sizes), value

        return self._on_map_plan(values, evidence_sets, sweep)

    def map_best(self, values, m, evidence=None):
        """The `m` most probable pairwise distinct joint assignments (1 <= m <= 16), best first: a list of ({variable: state},
        log_value), shorter than `m` where fewer assignments have a positive value; its first entry is what `map` returns.  One
        sweep on the device (`engine.Plan.map_best`) on the plan `map` makes - where clamping and re-running `map` along a partition
        of the assignments costs about m x cliques sweeps.  Evidence of probability zero raises `_capi.JtpError`, carrying `states`
        ({variable: int32 array of m times -1}) and `log_value` (-inf)."""
        sizes = self.clique_tree.factor_graph.sizes

        def sweep(plan):
            try:
                states, value = plan.map_best(m)
            except Exception as exc:
                if hasattr(exc, "states"):
                    exc.states = self._map_columns(plan, exc.states, sizes)
                raise
            cols = self._map_columns(plan, states, sizes)
            return [({lab: int(col[s]) for lab, col in cols.items()}, float(value[s])) for s in range(len(value))]

        return self._on_map_plan(values, [dict(evidence) if evidence else {}], sweep)

    def marginal_map(self, values, variables, evidence=None):
        """Marginal MAP (not in the reference): the most probable assignment of `variables` with every other variable summed out,
        ({variable: state} for those variables only, log_value) - log_value = log max_m sum_s prod of the factor values; less log Z
        it is the log posterior probability of that assignment.  `evidence`: {variable: observed state}.  `map` maximises over the
        other variables instead of summing them, which is another answer in general.  See `marginal_map_evidence_sets`."""
        states, value = self.marginal_map_evidence_sets(values, variables, [dict(evidence) if evidence else {}])
        return {lab: int(col[0]) for lab, col in states.items()}, float(value[0])

    def marginal_map_evidence_sets(self, values, variables, evidence_sets):
        """`marginal_map` for several evidence sets over the same factor values: ({variable: int32 array of length n_sets}, float64
        array of the sets' log values), all sets through the same launches of one sweep on the device (`engine.Plan.marginal_map`).

        Max and sum do not commute, so the sweep does not run on this tree but on a strong junction tree of the same factors
        built for the query (`construction.strong_junction_tree`: the summed variables eliminated first), remembered per set of
        query variables; the factor values apply to it as they are.  Its cliques can be far wider than this tree's - that is
        inherent to marginal MAP - and a clique beyond the engine's limits raises `_capi.UnsupportedStructure`.  Every clique
        table is materialised, as for `map`.  An empty query gives ({}, log Z).  A set whose evidence has probability zero raises
        `_capi.JtpError`, carrying `states` (-1 for that set) and `log_value` (-inf)."""
        from ._capi import UnsupportedStructure

        fg = self.clique_tree.factor_graph
        sizes = fg.sizes
        variables = list(variables)
        for lab in variables:
            if lab not in sizes:
                raise ValueError("variable %r is not a variable of the model" % (lab,))
        if len(set(variables)) != len(variables):
            raise ValueError("a variable is listed twice: %r" % (variables,))
        n_sets = len(evidence_sets)
        if n_sets == 0:
            return {lab: np.zeros(0, dtype=np.int32) for lab in variables}, np.zeros(0)
        memo = ("strong", frozenset(variables))
        mark = (tuple(sizes.items()), tuple(sorted(self._opts.items())))
        hit = self._memo.get(memo)
        if hit is None or hit[0] != mark:
            maxcliques, f2m, tree, separators = cons.strong_junction_tree(fg.factors, sizes, variables)
            strong = JunctionTree(tree=tree, separators=separators,
                                  clique_tree=CliqueGraph(maxcliques=maxcliques, factor_to_maxclique=f2m, factor_graph=fg), _opts=dict(self._opts))
            hit = self._memo[memo] = (mark, strong)
        strong = hit[1]

        def columns(known, states, value):
            got = dict(zip(known, states.T))
            rest = np.where(np.isneginf(value), -1, 0).astype(np.int32)     # (a variable of no factor has no state to choose: 0)
            return {lab: got.get(lab, rest) for lab in variables}

        def sweep(plan):
            known = [lab for lab in variables if lab in plan.var_id or lab in plan._trivial]
            try:
                states, value = plan.marginal_map(known, 0, n_sets)
            except Exception as exc:
                if hasattr(exc, "states"):
                    exc.states = columns(known, exc.states, exc.log_value)
                raise
            return columns(known, states, value), value

        try:
            return strong._on_map_plan(values, evidence_sets, sweep)
        except UnsupportedStructure as exc:
            raise UnsupportedStructure("%s - marginal MAP runs on a junction tree in which the summed variables are eliminated before the query variables, "
                                       "whose cliques can be far larger than those of the tree `propagate` uses" % exc) from exc

    def _on_map_plan(self, values, evidence_sets, sweep):
        """`sweep(plan)` on the plan the max-product calls share (`map_evidence_sets`, `max_propagate_evidence_sets`): one copy of the
        clique tables, an evidence set per entry of the non-empty `evidence_sets`; the factor values staged, the evidence set, and
        cleared again whatever happens."""
        import weakref
        from . import engine

        ct = self.clique_tree
        sizes = ct.factor_graph.sizes
        n_sets = len(evidence_sets)
        all_f32 = all(type(x) is np.ndarray and x.dtype == np.float32 for x in values)
        dtype = "f32" if all_f32 else "f64"
        # (an entry of its own, as `sample` keeps: what `propagate(xs, changed=...)` trusts about "plan" is never said of this plan)
        mark = (dtype, n_sets, tuple(sizes.items()), tuple(sorted(self._opts.items())))
        hit = self._memo.get("plan_map")
        plan = engine.cached_plan(hit[1], hit[2]()) if hit is not None and hit[0] == mark else None
        if plan is None:
            node_vars = [list(c) for c in ct.maxcliques] + [list(s) for s in self.separators]
            plan, key = engine.plan_for(self.tree, node_vars, sizes, dtype, return_key=True, n_batch=n_sets, share_potentials=True, **self._opts)
            self._memo["plan_map"] = (mark, key, weakref.ref(plan))
        _stage_changed_cliques(plan, ct, values)
        try:
            for b, observed in enumerate(evidence_sets):
                plan.set_evidence(dict(observed) if observed else {}, batch=b)
            return sweep(plan)
        finally:
            for b, observed in enumerate(evidence_sets):     # (the plan is the cache's: whoever is handed it next finds no evidence set)
                if observed:
                    plan.set_evidence({}, batch=b)

    def max_propagate(self, values, evidence=None):
        """Max-propagation (not in the reference): (list, log_value) - per factor a float64 array of the factor's shape holding the
        LOG of its unnormalised max-marginal: for every assignment of the factor's variables the log of the product of the factor
        values at the best full assignment that agrees with it and with `evidence` ({variable: observed state}); -inf where no
        assignment of positive value does.  Every array's maximum is `log_value`, the log value of the most probable assignment
        (`map`): an entry's distance below it says how much worse the best explanation gets when those variables are held there,
        and a variable whose max-marginal has two entries at the maximum has no unique most probable state.
        See `max_propagate_evidence_sets`."""
        tables, value = self.max_propagate_evidence_sets(values, [dict(evidence) if evidence else {}])
        return tables[0], float(value[0])

    def max_propagate_evidence_sets(self, values, evidence_sets):
        """`max_propagate` for several evidence sets over the same factor values: (one list of arrays per set, float64 array of the
        sets' log values), all sets through the same launches of one upward and one downward max-product sweep on the device
        (`engine.Plan.max_marginals`) - where clamping every variable to every state in turn costs sum(cardinalities) sweeps of
        `map`.  It runs on the plan `map_evidence_sets` makes (every clique table materialised).  The sweep rescales its messages by
        powers of two; the logarithm is np.log(table) + log2_scale * np.log(2.0), so models whose values lie beyond float64 need
        nothing special.  A set whose evidence has probability zero raises `_capi.JtpError`, carrying `max_marginals` (all -inf for
        that set) and `log_value` (-inf)."""
        ct = self.clique_tree
        n_sets = len(evidence_sets)
        if n_sets == 0:
            return [], np.zeros(0)
        requests = [(ct.factor_to_maxclique[f], list(labels)) for f, labels in enumerate(ct.factor_graph.factors)]

        def logs(tables, scale):
            with np.errstate(divide="ignore"):
                return [[np.log(t) + float(e) * np.log(2.0) for t, e in zip(tables[b], scale[b])] for b in range(n_sets)]

        def sweep(plan):
            try:
                tables, scale, value = plan.max_marginals(requests, 0, n_sets)
            except Exception as exc:
                if hasattr(exc, "tables"):
                    exc.max_marginals = logs(exc.tables, exc.log2_scale)
                raise
            return logs(tables, scale), value

        return self._on_map_plan(values, evidence_sets, sweep)

    def max_marginals(self, values, evidence=None):
        """{variable: float64 vector}: the log max-marginal of every variable - entry s is the log value of the best full
        assignment with the variable in state s (and `evidence` observed), -inf where there is none.  Taken on the host from one
        factor of `max_propagate` that holds the variable, by a maximum over its other axes: exact."""
        tables, _ = self.max_propagate(values, evidence)
        out = {}
        for labels, table in zip(self.clique_tree.factor_graph.factors, tables):
            for ax, lab in enumerate(labels):
                if lab not in out:
                    out[lab] = table.max(axis=tuple(a for a in range(table.ndim) if a != ax))
        return out

    @staticmethod
    def _map_columns(plan, states, sizes):
        out = {lab: states[:, j] for j, lab in enumerate(plan.var_labels)}
        zeros = np.where(states[:, :1].reshape(-1) < 0, -1, 0).astype(np.int32) if states.shape[1] else np.zeros(len(states), dtype=np.int32)
        for lab in plan._trivial:                            # (one-state variables the plan keeps on the host)
            out[lab] = zeros
        for lab in sizes:                                    # (variables of no clique cannot occur: every variable is in a factor)
            out.setdefault(lab, zeros)
        return out

    def propagate_evidence_sets(self, xs, evidence_sets, normalize=False):
        """`propagate` for several hard-evidence sets over the same factor values (no counterpart in the
        reference, whose users loop over `propagate` after slicing the factors, `README.md:155-165`):
        `evidence_sets` is a list of {variable: observed state}; returns one list of factor marginals
        per set, each factor with its full shape (entries contradicting the evidence are zero) and
        every table of set e summing to P(evidence e) * Z.  The clique tables are formed once and
        shared by all sets; a pass over a table serves eight sets at a time (JTP_MULTISET).

        `normalize`: the sets run on an overflow-safe plan (`engine.Plan(scaled=True, share_potentials=True)`: one pass per set
        over the shared tables - scaled multi-set plans are not built), every marginal is divided by its own sum, and
        `tree.log_z_sets[e]` is log|Z_e|: log P(evidence e) = log_z_sets[e] - that of a set observing nothing."""
        ct = self.clique_tree
        if not evidence_sets:
            return []
        plan = self._propagated_evidence_plan(xs, evidence_sets, normalize)
        if normalize:
            out = [_normalised(plan.factor_marginals(ct.factor_graph.factors, ct.factor_to_maxclique, batch=b)) for b in range(len(evidence_sets))]
            self._memo["log_z_sets"] = np.array([plan.log_z(batch=b)[1] for b in range(len(evidence_sets))])
            return out
        return [plan.factor_marginals(ct.factor_graph.factors, ct.factor_to_maxclique, batch=b) for b in range(len(evidence_sets))]

    def _propagated_evidence_plan(self, xs, evidence_sets, normalize):
        """The plan `propagate_evidence_sets` and `expected_counts` run a non-empty list of evidence sets on, with the factor values
        staged, the evidence set and every set propagated (enqueued, not waited for)."""
        from . import engine

        ct = self.clique_tree
        all_f32 = all(isinstance(x, np.ndarray) and x.dtype == np.float32 for x in xs)
        node_vars = [list(c) for c in ct.maxcliques] + [list(s) for s in self.separators]
        # one copy of the tables; eight evidence sets per pass over a table (JTP_MULTISET), marginals formed
        # on demand from the tables and each set's final messages
        from ._capi import UnsupportedStructure
        if normalize:
            plan = engine.plan_for(self.tree, node_vars, ct.factor_graph.sizes, "f32" if all_f32 else "f64",
                                   n_batch=len(evidence_sets), share_potentials=True, scaled=True, cover=self.cover(), **self._opts)
            plan.evidence_mode = "one pass per evidence set over shared tables (scaled plan: messages divided by powers of two)"
        else:
            try:
                plan = engine.plan_for(self.tree, node_vars, ct.factor_graph.sizes, "f32" if all_f32 else "f64",
                                       n_batch=len(evidence_sets), multiset=True, **self._opts)
                plan.evidence_mode = "multiset: eight evidence sets per pass over a table"
            except UnsupportedStructure as exc:
                # separators too large for the per-set LDS regions of a multi-set pass (e.g. 64 x 64 doubles): the sets
                # still share one copy of the tables but run one pass each, one HIP stream each - up to eight times the table traffic
                # of a multi-set plan, so it is said, not done silently (`plan.evidence_mode`, and a warning once per tree)
                import warnings
                plan = engine.plan_for(self.tree, node_vars, ct.factor_graph.sizes, "f32" if all_f32 else "f64",
                                       n_batch=len(evidence_sets), share_potentials=True, cover=self.cover(), **self._opts)
                plan.evidence_mode = "one pass per evidence set over shared tables (the multi-set plan was refused: %s)" % exc
                if not self._memo.get("warned_multiset"):
                    self._memo["warned_multiset"] = True
                    warnings.warn("junctiontree_amd: the evidence sets of this tree run one pass each instead of eight per pass (%s)" % exc,
                                  RuntimeWarning, stacklevel=3)
        self._memo["evidence_plan"] = plan
        _stage_changed_cliques(plan, ct, xs)
        for b, observed in enumerate(evidence_sets):
            plan.set_evidence(observed, batch=b)
        plan.propagate(0, len(evidence_sets))
        return plan

    def expected_counts(self, values, evidence_sets, weights=None, normalize=False):
        """The E-step of EM (not in the reference): one float64 array per factor, of the factor's shape, holding
        sum_e weights[e] * P(the factor's variables | evidence set e) - every set's factor marginal divided by its own sum, added up
        on the device (`engine.Plan.accumulate_marginals`: nothing but the sums crosses to the host).  `evidence_sets` as in
        `propagate_evidence_sets` (one {variable: observed state} per data case), `weights` None: all 1.

        `tree.log_z_sets[e]` is then log|Z_e|, whatever the weight: add `{}` as one more set with weight 0 to obtain log Z of the
        model without evidence, and hence log P(evidence e) = log_z_sets[e] - log_z_sets[-1], the terms of the data log-likelihood.
        The plan is chosen as `propagate_evidence_sets` chooses it (`normalize`: the overflow-safe plan).  A set whose evidence has
        probability zero contributes nothing; `_capi.JtpError` is raised, carrying the sums of the other sets as `counts` and the
        logarithms as `log_z`.  The sums are counts for non-negative factor values only."""
        ct = self.clique_tree
        n_sets = len(evidence_sets)
        if weights is not None:
            weights = np.asarray(weights, dtype=np.float64).reshape(-1)
            if len(weights) != n_sets:
                raise ValueError("%d weights for %d evidence sets" % (len(weights), n_sets))
            if not np.isfinite(weights).all():
                raise ValueError("weights must be finite")
        if n_sets == 0:
            self._memo["log_z_sets"] = np.zeros(0)
            return [np.zeros(np.shape(x), dtype=np.float64) for x in values]
        plan = self._propagated_evidence_plan(values, evidence_sets, normalize)
        try:
            out, log_z, _ = plan.factor_counts(ct.factor_graph.factors, ct.factor_to_maxclique, weights=weights, batch_begin=0, batch_end=n_sets)
        except Exception as exc:
            if hasattr(exc, "log_z"):
                self._memo["log_z_sets"] = np.array(exc.log_z)
            raise
        self._memo["log_z_sets"] = np.array(log_z)
        return out
