"""Signed tables for the tests, and the bound a result on them is held to (tests/test_signed_emulated.py on the CPU,
tests/test_gpu_signed.py on the device).

The reference's own tests draw `randn` potentials, so tables with negative entries are part of the contract.  A belief entry is a
sum of products of table entries; computed in any order it differs from the exact value by at most a small multiple of eps times the
same sum over the ABSOLUTE values.  So with

    B_abs = oracle.beliefs_exact(tree, [abs(p) for p in pots], node_vars),    Z_abs its z

every entry is checked as |got - want| <= rtol * B_abs + 1e-300, rtol the project's constants (1e-11 float64 storage, 1e-6 float32
storage, `want` and `B_abs` then from the float32-cast tables); a marginal against the same marginal of B_abs, z against rtol * Z_abs.
On non-negative tables B_abs == want: exactly the elementwise tolerance of the other tests, nothing wider, no entry left out.

The bound says something only where cancellation is mild, so every case first asserts, on the oracle alone (`conditions`):
    kappa = B_abs / |want| over every belief entry (cliques and separators) that can be non-zero: median <= 100, max <= 1e4
        (a wrong index moves an entry by a few per cent of |want| or more: six orders above 1e-11 x 1e4, one above 1e-6 x 1e4)
    at least 5 % of those entries are negative.
Plain `randn` tables miss the first condition on anything but toy trees (the answer drowns in rounding).

Generator (`signed_potentials`): `synthetic.potentials_for(spec, seed)` with the sign of every clique-table entry flipped
independently with probability 1/8, the flips from `numpy.random.default_rng(seed + 1000)` clique after clique (one `random` call of
the table's shape each, flipped where it is below 1/8).  Magnitudes stay, so the float32 cast of a table is the cast of its
magnitudes.  A term of a belief is a product of one entry per clique, so the expected cancellation grows like 0.75^-n_cliques:
15 cliques is where the conditions still hold (a 31-clique width-15 tree sits at a median kappa of 5,700 and a rate of 1/4 breaks
them on most specs).

At rate 1/8 messages of long sums stay positive, so every family also runs the same tables with one leaf clique negated
(`negated`): the joint changes sign - Z < 0, the separator belief of the leaf's edge nowhere positive (asserted on the oracle by
`negation_facts`: the message really is negative) - and with an inner clique negated as well, Z > 0 again.  B_abs is the same for
all three.

Measured with the oracle on the CPU (seed 21, float64 tables; the float32 casts give the same figures to three digits; median kappa,
max kappa, negative share over all clique and separator beliefs); the leaf negations leave kappa as it is and turn the share into
its complement:
    wide_binary_tree(15, 14, 7, seed 2)                    54.8    131     0.124
    random_tree(9, 13, 5, seed 3)                          9.81    16.4    0.124
    chain_tree(6, card 16)                                 4.28    124     0.120
    wide_binary_tree(7, 8, 4, card 3, seed 3)              5.56    13.8    0.124
    wide_binary_tree(7, 6, 3, card 5, seed 5)              5.54    11.4    0.123
    wide_binary_tree(7, 5, 2, card 6, seed 6)              5.54    10.2    0.124
    (emulator only) chain_tree(5, card 4)                  3.27    177     0.154
    (emulator only) random_tree(8, 4, 2, card 5, seed 6)   7.11    68.4    0.115
    (scaled emulator) wide_binary_tree(7, 12, 6)           5.62    13.5    0.124
    the 15-clique tree under the six evidence sets         <= 55.4 <= 146  >= 0.123
    the card-3 tree under the six evidence sets            <= 5.81 <= 738  >= 0.123
    the trees of the expected-counts cases, per set        <= 56.1 <= 167  >= 0.123
    lattice_mrf(3, 6, 8), flips in every third factor      9.4     5,590   0.060      (factor marginals; flips in all 27 factors: 2,430 / 7.9e6)
Every case prints its own figures before anything is asserted (`pytest -s`), and `check` reports through `Bound.worst` how far below
the bound a result lies: on the MI355X the worst of any case was 4.1e-5 of the bound with float64 storage and 0.024 of it with
float32 storage (the rounding of a belief stored as float32).  Not measured: specs other than these, and seeds other than 21.
"""
import numpy as np

import jt_oracle as oracle

RTOL = {"f64": 1e-11, "f32": 1e-6}
FLIP_RATE = 0.125
KAPPA_MEDIAN, KAPPA_MAX, NEGATIVE_SHARE = 100.0, 1e4, 0.05


def flip_signs(arrays, seed, rate=FLIP_RATE):
    """`arrays` with the sign of every entry flipped independently with probability `rate` (a seeded generator, one draw per array)"""
    rng = np.random.default_rng(seed + 1000)
    out = []
    for a in arrays:
        a = np.asarray(a)
        out.append(np.where(rng.random(a.shape) < rate, -a, a).astype(a.dtype))
    return out


def signed_potentials(spec, seed=21, dtype=np.float64, rate=FLIP_RATE):
    """`synthetic.potentials_for(spec, seed, dtype)` with signs flipped in the clique tables (separators stay all ones)"""
    from junctiontree_amd import synthetic
    pots = synthetic.potentials_for(spec, seed=seed, dtype=dtype)
    n = spec["n_cliques"]
    return flip_signs(pots[:n], seed, rate) + pots[n:]


def negated(pots, cliques):
    """the same tables with every entry of the cliques named negated"""
    return [-np.asarray(p) if c in cliques else p for c, p in enumerate(pots)]


def leaf_and_inner(spec):
    """(a leaf clique, an inner clique that is neither the root nor that leaf's parent where the tree has one) of a recipe's spec"""
    parent = spec["parent"]
    n = spec["n_cliques"]
    has_child = {p for p in parent if p >= 0}
    leaf = max(c for c in range(n) if c not in has_child)
    inner = [c for c in sorted(has_child) if c != 0 and c != parent[leaf]] or [c for c in sorted(has_child) if c != 0] or [0]
    return leaf, inner[0]


class Bound:
    """The oracle's beliefs of signed tables (`want`, `z`) and of their absolute values (`b_abs`, `z_abs`), float64, computed once per
    case and left unchanged."""

    def __init__(self, tree, pots, node_vars, what=""):
        held = [np.asarray(p, dtype=np.float64) for p in pots]           # (float32 storage: the cast tables, widened)
        self.want, self.z = oracle.beliefs_exact(tree, held, node_vars, return_z=True)
        self.b_abs, self.z_abs = oracle.beliefs_exact(tree, [np.abs(p) for p in held], node_vars, return_z=True)
        self.node_vars = node_vars
        self.what = what
        self.worst = 0.0                                     # the largest |got - want| / (rtol * B_abs) any check of this case has seen
        for a in self.want + self.b_abs:
            a.setflags(write=False)

    # ---------------------------------------------------------------- conditions on the oracle alone
    def kappa(self):
        """B_abs / |want| over every belief entry that can be non-zero (entries hard evidence removes are zero on both sides)"""
        w = np.concatenate([np.ravel(a) for a in self.want])
        b = np.concatenate([np.ravel(a) for a in self.b_abs])
        live = b > 0
        with np.errstate(divide="ignore"):
            return b[live] / np.abs(w[live]), w[live]

    def conditions(self, negative_share=NEGATIVE_SHARE):
        k, w = self.kappa()
        med, mx, neg = float(np.median(k)), float(np.max(k)), float(np.mean(w < 0))
        print("%s: kappa median %.3g max %.3g, negative share %.3f, z %.6g" % (self.what, med, mx, neg, self.z))
        assert med <= KAPPA_MEDIAN and mx <= KAPPA_MAX, "%s: cancellation too strong for the bound to be sharp (kappa median %g, max %g)" % (self.what, med, mx)
        assert neg >= negative_share, "%s: only %.3f of the belief entries are negative" % (self.what, neg)
        return med, mx, neg

    # ---------------------------------------------------------------- comparisons
    def check(self, node, got, rtol, what=""):
        self.worst = max(self.worst, check(got, self.want[node], self.b_abs[node], rtol, "%s %s node %d" % (self.what, what, node)))

    def check_z(self, got, rtol, what=""):
        assert abs(got - self.z) <= rtol * self.z_abs, "%s %s: z %r, want %r (bound %g)" % (self.what, what, got, self.z, rtol * self.z_abs)

    def marginal(self, node, labels):
        """(want, bound table) of the marginal of node `node` onto `labels`, in that axis order"""
        axes = list(self.node_vars[node])
        return (oracle.labelled_einsum(self.want[node], axes, list(labels)), oracle.labelled_einsum(self.b_abs[node], axes, list(labels)))

    def check_marginal(self, node, labels, got, rtol, what=""):
        want, b_abs = self.marginal(node, labels)
        self.worst = max(self.worst, check(got, want, b_abs, rtol, "%s %s marginal of node %d onto %r" % (self.what, what, node, list(labels))))


def check(got, want, b_abs, rtol, what=""):
    """|got - want| <= rtol * B_abs + 1e-300 on every entry; returns the largest |got - want| / (rtol * B_abs + 1e-300) seen"""
    got = np.asarray(got, dtype=np.float64)
    want = np.broadcast_to(np.asarray(want, dtype=np.float64), got.shape)
    b_abs = np.broadcast_to(np.asarray(b_abs, dtype=np.float64), got.shape)
    assert np.all(np.isfinite(got)), what + ": not finite"
    err = np.abs(got - want)
    bad = err > rtol * b_abs + 1e-300
    if np.any(bad):
        i = tuple(int(x) for x in np.unravel_index(int(np.argmax(err / (b_abs + 1e-300))), got.shape)) if got.ndim else ()
        raise AssertionError("%s: %d of %d entries beyond %g x B_abs; worst at %r: got %r want %r B_abs %r"
                             % (what, int(bad.sum()), bad.size, rtol, i, got[i], want[i], b_abs[i]))
    return float(np.max(err / (rtol * b_abs + 1e-300))) if err.size else 0.0


def negation_facts(spec, pots, what=""):
    """The three inputs of a family - as generated, one leaf clique negated, an inner clique negated as well - as `Bound`s, with the
    facts about the negations asserted on the oracle: the separator belief of the negated leaf's edge is nowhere positive (and
    somewhere negative: the message that crosses it is negative), Z < 0 with one negation and Z > 0 with two."""
    n = spec["n_cliques"]
    leaf, inner = leaf_and_inner(spec)
    sep = n + leaf - 1                                   # (the recipes number the separator above clique c as n + c - 1)
    plain = Bound(spec["tree"], pots, spec["node_vars"], what)
    one = Bound(spec["tree"], negated(pots, {leaf}), spec["node_vars"], what + " leaf %d negated" % leaf)
    two = Bound(spec["tree"], negated(pots, {leaf, inner}), spec["node_vars"], what + " cliques %d and %d negated" % (leaf, inner))
    for b in (plain, one, two):
        b.conditions()
    assert np.all(one.want[sep] <= 0) and np.any(one.want[sep] < 0), "%s: the separator belief above the negated leaf is positive somewhere" % what
    assert one.z < 0 < two.z and plain.z > 0, (what, plain.z, one.z, two.z)
    return {"plain": (pots, plain), "leaf": (negated(pots, {leaf}), one), "leaf+inner": (negated(pots, {leaf, inner}), two)}, leaf, inner


# ------------------------------------------------------------------------------------------------ factor graphs (public API)

def signed_factors(values, seed=21, every=3):
    """Factor tables with signs flipped at rate 1/8 in every `every`-th factor (the others stay positive).  A term of a marginal is a
    product of one entry per FACTOR, so flips in all 27 factors of the 3 x 6 lattice cancel like 0.75^-27 (median kappa ~ 2,400 on
    the CPU, beyond the condition); in nine of them the median stays near 0.75^-9 = 13."""
    picked = list(range(0, len(values), every))
    flipped = flip_signs([values[i] for i in picked], seed)
    out = list(values)
    for i, v in zip(picked, flipped):
        out[i] = v
    return out


class FactorBound:
    """`oracle.propagate` of a factor graph on signed factor values and on their absolute values: the factor marginals `want` and
    their bound `b_abs`; Z = the sum of any of them."""

    def __init__(self, tree, factors, sizes, values, what=""):
        ct = tree.clique_tree
        vals = [np.asarray(v, dtype=np.float64) for v in values]
        args = (tree.tree, tree.separators, ct.maxcliques, ct.factor_to_maxclique, factors, sizes)
        self.want = oracle.propagate(*args, vals)
        self.b_abs = oracle.propagate(*args, [np.abs(v) for v in vals])
        self.z, self.z_abs = float(self.want[0].sum()), float(self.b_abs[0].sum())
        self.what = what

    def conditions(self, negative_share=NEGATIVE_SHARE):
        w = np.concatenate([np.ravel(a) for a in self.want])
        b = np.concatenate([np.ravel(a) for a in self.b_abs])
        with np.errstate(divide="ignore"):
            k = b / np.abs(w)
        med, mx, neg = float(np.median(k)), float(np.max(k)), float(np.mean(w < 0))
        print("%s: kappa median %.3g max %.3g, negative share %.3f, z %.6g" % (self.what, med, mx, neg, self.z))
        assert med <= KAPPA_MEDIAN and mx <= KAPPA_MAX, "%s: cancellation too strong (kappa median %g, max %g)" % (self.what, med, mx)
        assert neg >= negative_share, "%s: only %.3f of the marginal entries are negative" % (self.what, neg)
        return med, mx, neg

    def check(self, got, rtol, what=""):
        assert len(got) == len(self.want)
        for f, (g, w, b) in enumerate(zip(got, self.want, self.b_abs)):
            check(g, w, b, rtol, "%s %s factor %d" % (self.what, what, f))
