"""CPU emulation of JTP_SCALED plans, for tests only: tests/emulator.py with the kind-2 steps of the step list (`rescale` records:
every copy of one message as its consumers read it, divided by one power of two) executed with numpy by the rule of the kernel
`jt_rescale_level` (csrc/jtp_propagate.hip), clamps included, and the node exponents walked down the planner's tree the way the
engine's read-out does."""
import numpy as np

from emulator import Emulator


def message_exponent(values):
    """e of one message: the largest biased exponent field of its entries - 1023, clamped to [-1022, 1022]; 0 where that field is
    0 (all zero or subnormal) or 0x7ff (an inf or NaN somewhere)."""
    bits = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    field = int(((bits >> np.uint64(52)) & np.uint64(0x7FF)).max()) if bits.size else 0
    if field in (0, 0x7FF):
        return 0
    return int(min(max(field - 1023, -1022), 1022))


class ScaledEmulator(Emulator):
    def __init__(self, desc, rescale=True):
        super().__init__(desc)
        assert desc.get("scaled") == 1 and not desc["segments"] and not desc["flow_steps"]
        self.rescale = rescale                     # False: the same plan run without its kind-2 steps (the unscaled propagate)
        self.check_written = True                  # (cleared by tests whose values overflow on purpose: inf x 0 is a NaN too)
        self.exps = np.zeros(2 * len(desc["pseps"]), dtype=np.int64)

    def propagate(self, comm=None):
        """`Emulator.propagate` with the kind-2 steps; the launches are checked as there."""
        d = self.d
        self.msg[:] = np.nan
        self.exps[:] = 0
        self._init_blocks()
        for kind, first, count in d["steps"]:
            assert kind in (0, 2), "a scaled plan runs on one rank"
            if kind == 2:
                for rec in d["rescale"][first:first + count]:
                    buf = self.msg[rec["off"]:rec["off"] + rec["count"]]
                    # (every entry of every copy is written by then: the unwritten marker is a NaN and would switch the scaling off)
                    assert not (self.check_written and np.any(np.isnan(buf))), "a rescale step precedes a producer of its message"
                    if self.rescale:
                        e = message_exponent(buf)
                        self.exps[rec["slot"]] = e
                        if e:
                            buf *= np.ldexp(1.0, -e)
                continue
            launch = d["launches"][first]
            blocks = d["blocks"][launch["blk_off"]:launch["blk_off"] + launch["nblocks"]]
            assert not any(b[23] & 8 for b in blocks)
            seen = set()
            for blk in blocks:
                t, chunk = blk[0], blk[1]
                tk = d["tasks"][t]
                assert t in launch["tasks"] and launch["variant"] in (tk["variant"], 12 + launch["phase"])
                assert tk["lds_bytes"] <= launch["lds_bytes"]
                seen.add((t, chunk))
                self._block(tk, chunk, tk["mode"] == 0, blk[2:])
            assert all(not ((t, c) in seen) for t in launch["tasks"] for c in self._init_seen.get(t, ()))
            assert len(seen) == len(blocks) == sum((1 << d["tasks"][t]["nF"]) - len(self._init_seen.get(t, ())) for t in launch["tasks"])
        self._check_unit_counts()

    def node_exponents(self):
        """(E per planner node, E per separator): what the emulated arenas hold for a node is its true table x 2^-E.
        E_root = the sum of every e_up; E_child = E_parent - e_up(child) + e_dn(child); a separator: E_parent + e_dn(child)."""
        pn = self.d["pnodes"]
        node_e, sep_e = [0] * len(pn), [0] * len(self.d["pseps"])
        all_up = sum(int(self.exps[2 * p["psep"]]) for p in pn if p["psep"] >= 0)
        for c in sorted(range(len(pn)), key=lambda c: pn[c]["depth"]):
            p = pn[c]
            if p["psep"] < 0:
                node_e[c] = all_up
                continue
            sep_e[p["psep"]] = node_e[p["parent"]] + int(self.exps[2 * p["psep"] + 1])
            node_e[c] = sep_e[p["psep"]] - int(self.exps[2 * p["psep"]])
        return node_e, sep_e
