"""Hard evidence as the reference defines it: slicing (reference `computation.py:11-34`, `README.md:155-165`).

The observed state is cut out of EVERY table that holds the variable, so an entry that contradicts the evidence is never
read - whatever it holds.  `sliced_beliefs` does that on a tree of clique tables and embeds the results back into the full
shapes (zeros elsewhere); `poison` writes a value of the caller's choice into every contradicted entry, which must not change
one bit of any result.  The same pair over a factor list, for the public API: `sliced_factor_marginals`, `poison_factors`.

The older evidence tests multiply a one-hot indicator into ONE clique and run the oracle on that: equal to slicing while every
entry is finite, NaN as soon as a contradicted entry is `inf` or NaN (0 x inf).  numpy only."""
import numpy as np

import jt_oracle as oracle

# what a contradicted entry may hold: non-finite values, and a finite one whose product with itself overflows float64
# ("big": float64 storage only - float32 staging turns it into inf)
KINDS = {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan, "big": 1e200}


def _contradicted(labels, shape, observed):
    """Boolean array of `shape`: True where the index disagrees with `observed` on some axis."""
    bad = np.zeros(shape, dtype=bool)
    for ax, lab in enumerate(labels):
        if lab in observed:
            off = np.arange(shape[ax]) != observed[lab]
            bad |= off.reshape([-1 if a == ax else 1 for a in range(len(shape))])
    return bad


def _slice(table, labels, observed):
    for ax, lab in enumerate(labels):
        if lab in observed:
            table = np.take(table, [observed[lab]], axis=ax)
    return table


def _embed(table, labels, shape, observed):
    full = np.zeros(shape, dtype=np.float64)
    full[tuple(slice(observed[lab], observed[lab] + 1) if lab in observed else slice(None) for lab in labels)] = table
    return full


def node_tables(spec, pots):
    """`pots` as float64 arrays over the whole node list (separators that the caller left out: ones - their values are unused)."""
    node_vars = spec["node_vars"]
    out = [np.asarray(p, dtype=np.float64) for p in pots]
    out += [np.ones([spec["sizes"][v] for v in node_vars[n]]) for n in range(len(out), len(node_vars))]
    return out


def sliced_beliefs(spec, pots, observed):
    """(beliefs, Z): the oracle on tables with the observed states cut out of every node table that holds the variable, every
    belief embedded into its node's full shape with zeros at the contradicted entries."""
    node_vars = spec["node_vars"]
    full = node_tables(spec, pots)
    cut = [_slice(t, node_vars[n], observed) for n, t in enumerate(full)]
    beliefs, z = oracle.beliefs_exact(spec["tree"], cut, node_vars, return_z=True)
    return [_embed(b, node_vars[n], full[n].shape, observed) for n, b in enumerate(beliefs)], z


def indicator_beliefs(spec, pots, observed):
    """(beliefs, Z) of the older tests' reference: a one-hot indicator multiplied into the first clique that holds the variable."""
    node_vars = spec["node_vars"]
    tabs = node_tables(spec, pots)
    for var, state in observed.items():
        host = next(c for c in range(spec["n_cliques"]) if var in node_vars[c])
        ind = np.zeros(spec["sizes"][var])
        ind[state] = 1.0
        ax = node_vars[host].index(var)
        tabs[host] = tabs[host] * ind.reshape([-1 if a == ax else 1 for a in range(tabs[host].ndim)])
    return oracle.beliefs_exact(spec["tree"], tabs, node_vars, return_z=True)


def poison(spec, pots, observed, kind):
    """A copy of the clique tables (dtypes kept) with every entry that contradicts `observed`, in every clique that holds an
    observed variable, set to KINDS[kind]."""
    out = []
    for c in range(spec["n_cliques"]):
        t = np.array(pots[c])
        t[_contradicted(spec["node_vars"][c], t.shape, observed)] = KINDS[kind]
        out.append(t)
    return out + [np.array(p) for p in pots[spec["n_cliques"]:]]


def poisoned_fraction(spec, observed):
    """Per clique, the share of its entries that `poison` overwrites."""
    return [float(_contradicted(spec["node_vars"][c], [spec["sizes"][v] for v in spec["node_vars"][c]], observed).mean())
            for c in range(spec["n_cliques"])]


def holders(spec, var):
    return [c for c in range(spec["n_cliques"]) if var in spec["node_vars"][c]]


# ---------------------------------------------------------------------------------------- factor lists (the public API)

def sliced_factor_marginals(tree, factors, sizes, values, observed):
    """The factor marginals of `tree.propagate` under `observed`, by slicing: the observed state cut out of every factor that holds
    the variable and its size set to 1 (what the reference's users do), the oracle's propagate over the junction tree `tree`, every
    marginal embedded into the factor's full shape.  Every returned table sums to P(observed) * Z."""
    ct = tree.clique_tree
    cut_sizes = {v: (1 if v in observed else n) for v, n in sizes.items()}
    cut = [_slice(np.asarray(x, dtype=np.float64), f, observed) for f, x in zip(factors, values)]
    out = oracle.propagate(tree.tree, tree.separators, ct.maxcliques, ct.factor_to_maxclique, factors, cut_sizes, cut)
    return [_embed(np.asarray(o, dtype=np.float64), f, np.shape(x), observed) for o, f, x in zip(out, factors, values)]


def poison_factors(factors, values, observed, kind, zeros=()):
    """A copy of the factor tables with every entry that contradicts `observed` set to KINDS[kind] - and to 0 in the factors listed
    in `zeros`: the product a clique table is formed from then holds 0 x inf = NaN at such an entry."""
    out = []
    for i, (f, x) in enumerate(zip(factors, values)):
        t = np.array(x)
        t[_contradicted(f, t.shape, observed)] = 0.0 if i in zeros else KINDS[kind]
        out.append(t)
    return out


def bits(a):
    """The bit patterns of a float array: equality of these sees a NaN that `==` would not and tells -0 from 0."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---------------------------------------------------------------------------------------- the cases host and device tests share

def widest_clique(spec):
    return max(range(spec["n_cliques"]), key=lambda c: (len(spec["node_vars"][c]), -c))


def sweep_sets(spec, n_single=None, seed=0, total=None):
    """Evidence sets that put a mask on every kind of index bit of one table in turn: set 0 observes nothing, set k the k-th
    variable of the widest clique (`n_single` of them, spread evenly from the first to the last where that is fewer than the
    clique has), then two sets of three variables of which two share a clique - and, up to `total` sets, sets of two variables of
    one clique further down.  States are drawn from `seed`."""
    rng = np.random.default_rng(seed)
    nv, n = spec["node_vars"], spec["n_cliques"]
    wide = nv[widest_clique(spec)]
    k = len(wide) if n_single is None else min(n_single, len(wide))
    picks = [wide[int(round(i))] for i in np.linspace(0, len(wide) - 1, k)]
    state = lambda v: int(rng.integers(0, spec["sizes"][v]))
    sets = [{}] + [{v: state(v)} for v in picks]
    last, first = nv[n - 1], nv[0]
    for pair, other in (((last[0], last[-1]), first), ((first[0], first[-1]), last[::-1])):
        third = next(v for v in other if v not in pair)
        sets.append({v: state(v) for v in pair + (third,)})
    c = 1
    while total is not None and len(sets) < total:
        sets.append({v: state(v) for v in (nv[c][1], nv[c][-2])})
        c += 1
    return sets


def tree_cases():
    """name -> (spec, storage dtype, evidence sets): the trees of the device tests, the smallest of today's suite that reach each path."""
    from junctiontree_amd import synthetic
    out = {}
    spec = synthetic.wide_binary_tree(n_cliques=7, width=13, sep=6, card=2, seed=6)
    out["pow2_f64"] = (spec, "f64", sweep_sets(spec))                 # 1 + 13 + 2 sets: element, lane, loop and chunk bits
    out["pow2_f32"] = (spec, "f32", sweep_sets(spec))
    for card, width, sep in ((3, 8, 4), (5, 6, 3)):
        spec = synthetic.wide_binary_tree(n_cliques=7, width=width, sep=sep, card=card, seed=3)
        for dt in ("f64", "f32"):
            out["card%d_%s" % (card, dt)] = (spec, dt, sweep_sets(spec))
    # multi-set plans: 11 sets - a padded last group
    spec = synthetic.wide_binary_tree(n_cliques=15, width=13, sep=6, card=2, seed=2)
    out["multi_pow2_f64"] = (spec, "f64", sweep_sets(spec, n_single=8, total=11))
    spec = synthetic.wide_binary_tree(n_cliques=7, width=14, sep=7, card=2, seed=6)
    out["multi_pow2_f32"] = (spec, "f32", sweep_sets(spec, n_single=8, total=11))
    spec = synthetic.random_tree(n_cliques=9, width=6, sep=3, card=3, seed=4)
    out["multi_card3_f64"] = (spec, "f64", sweep_sets(spec, n_single=8, total=11))
    return out


def kinds_for(dtype):
    return ["+inf", "-inf", "nan"] + (["big"] if dtype == "f64" else [])


def clean_tables(spec, dtype, seed=4):
    from junctiontree_amd import synthetic
    return synthetic.potentials_for(spec, seed=seed, dtype=np.float32 if dtype == "f32" else np.float64)


def zero_partners(factors, factor_to_clique, observed):
    """Factors to hand `poison_factors` as `zeros`: where two factors of one clique hold the same observed variable, the second."""
    out = set()
    for var in observed:
        by_clique = {}
        for i, f in enumerate(factors):
            if var in f:
                by_clique.setdefault(factor_to_clique[i], []).append(i)
        out.update(group[1] for group in by_clique.values() if len(group) >= 2 and group[0] not in out)
    return out
