"""numpy reference for expected counts (`jtp_accumulate_marginals`, `engine.Plan.accumulate_marginals`, `JunctionTree.expected_counts`):
the oracle's exact beliefs on indicator-multiplied potentials, one evidence set after the other, every requested marginal divided by
its own sum and added with the set's weight.  `tests/test_counts_host.py` pins it against a brute-force joint."""
import numpy as np

import jt_oracle as oracle


def full_potentials(spec, potentials):
    """Clique potentials at their full shapes (length-1 axes broadcast), followed by separators of ones."""
    n = spec["n_cliques"]
    out = []
    for c in range(n):
        shape = [spec["sizes"][v] for v in spec["node_vars"][c]]
        out.append(np.broadcast_to(np.asarray(potentials[c], dtype=np.float64), shape).copy())
    out += [np.ones([spec["sizes"][v] for v in labs]) for labs in spec["node_vars"][n:]]
    return out


def indicator_potentials(spec, base, observed):
    """`base` with the indicator of every observed variable multiplied into one clique that holds it (the recipe of
    `tests/test_gpu_parity.py`)."""
    pots = [np.asarray(p, dtype=np.float64).copy() for p in base]
    for var, state in observed.items():
        host = next(c for c in range(spec["n_cliques"]) if var in spec["node_vars"][c])
        ind = np.zeros(spec["sizes"][var])
        ind[state] = 1.0
        shape = [1] * pots[host].ndim
        shape[spec["node_vars"][host].index(var)] = spec["sizes"][var]
        pots[host] = pots[host] * ind.reshape(shape)
    return pots


def expected_counts_reference(spec, potentials, requests, evidence_sets, weights=None):
    """(counts, log_z): counts[i] = sum_e weights[e] * m_ei / sum(m_ei), m_ei the marginal of clique requests[i][0]'s belief under
    evidence set e onto the labels requests[i][1] (in that axis order); log_z[e] = log|Z_e|.  A set of weight 0 is left out of the
    sums whatever it holds; so is a (set, request) pair whose marginal sums to zero."""
    base = full_potentials(spec, potentials)
    weights = np.ones(len(evidence_sets)) if weights is None else np.asarray(weights, dtype=np.float64)
    counts = [np.zeros([spec["sizes"][v] for v in labels]) for _, labels in requests]
    log_z = np.zeros(len(evidence_sets))
    for e, observed in enumerate(evidence_sets):
        beliefs, z = oracle.beliefs_exact(spec["tree"], indicator_potentials(spec, base, observed), spec["node_vars"], return_z=True)
        with np.errstate(divide="ignore"):
            log_z[e] = np.log(abs(z))
        if weights[e] == 0:
            continue
        for i, (c, labels) in enumerate(requests):
            m = oracle.labelled_einsum(beliefs[c], list(spec["node_vars"][c]), list(labels))
            total = m.sum()
            if total != 0 and np.isfinite(total):
                counts[i] += weights[e] * (m / total)
    return counts, log_z


def bruteforce_counts(spec, potentials, requests, evidence_sets, weights=None):
    """The same from the full joint: one einsum over all variables per evidence set (small models only)."""
    base = full_potentials(spec, potentials)[:spec["n_cliques"]]
    weights = np.ones(len(evidence_sets)) if weights is None else np.asarray(weights, dtype=np.float64)
    variables = sorted(spec["sizes"])
    ops = []
    for c in range(spec["n_cliques"]):
        ops += [base[c], list(spec["node_vars"][c])]
    joint = oracle.labelled_einsum(*ops, variables)
    counts = [np.zeros([spec["sizes"][v] for v in labels]) for _, labels in requests]
    log_z = np.zeros(len(evidence_sets))
    for e, observed in enumerate(evidence_sets):
        j = joint
        for var, state in observed.items():
            ind = np.zeros(spec["sizes"][var])
            ind[state] = 1.0
            j = j * ind.reshape([-1 if v == var else 1 for v in variables])
        with np.errstate(divide="ignore"):
            log_z[e] = np.log(abs(j.sum()))
        if weights[e] == 0:
            continue
        for i, (_, labels) in enumerate(requests):
            m = oracle.labelled_einsum(j, variables, list(labels))
            if m.sum() != 0:
                counts[i] += weights[e] * (m / m.sum())
    return counts, log_z
