"""The decisions of the convolution launch planner (codd_amd/ops.py) that tests/golden/conv_plan_bits.json records, shared by
the generator tools/parent_bits.py --cases conv_plan and by tests/test_conv_plan_bits.py.  No device: the planner asks the
library's dry runs only, the layers are stubs with the fields of a PackedConv the planner reads, and the ConvParams are
built from the signature (the formats: the comment above ops._plain_key; conv_fp64.parse_sig reads them).  A digest is
sha256 over the canonical JSON of what a key hashes:

* ``db/<signature>``: every signature of codd_amd/tuned/mi355x.json.
    fp32          the _conv_cfg pick; the candidate list (and the log description) _autotune hands to _time_cfgs, which a
                  recorder replaces: nothing is timed or launched
    b<terms>|...  the candidates the library accepts (_bf16_candidates filtered by _cfg_ok), as they are and through
                  _small_footprint; _split_dims of the first one and of the whole list; the _conv_cfg pick the
                  split-or-fp32 choice falls back to
    g<gate>,...   the accepted candidates, through _small_footprint for gate 1
* ``grid/<signature>``: small layers the db does not hold -- cin 3 | 9 | 196, cout 16 | 18 | 576, 1x1 | 7x7 stride 2 |
  3x3 dilation 2, maps 7x30 | 9x21 | 72x120, B 1 | 2 -- hashed as an fp32 AND as a b3 signature.
* ``split_rows/1..300``: _split_rows(H) for H = 1 ... 300.

Only functions whose names and signatures the planner keeps are called (_conv_cfg, _autotune, _time_cfgs, _bf16_candidates,
_cfg_ok, _small_footprint, _split_dims, _split_rows, _set_cfg), so this file runs unchanged in a checkout of the commit
before a change of the planner: that is how the fixture is made."""
import hashlib
import itertools
import json
import os

from conv_fp64 import parse_sig

NAME = "conv_plan"
SOURCES = ("codd_amd/ops.py", "codd_amd/csrc/conv.hip", "codd_amd/csrc/conv_bf16.hip")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DB = os.path.join(ROOT, "codd_amd", "tuned", "mi355x.json")

GRID_CIN, GRID_COUT = (3, 9, 196), (16, 18, 576)
GRID_KERNELS = ((1, 1, 1, 0), (7, 2, 1, 3), (3, 1, 2, 2))  # (k, stride, dilation, pad)
GRID_MAPS, GRID_B = ((7, 30), (9, 21), (72, 120)), (1, 2)


def digest(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


class Layer:
    """The fields of a PackedConv the planner reads."""

    def __init__(self, cout_eff, cin, kh, kw, mb, deconv):
        self.cout_eff, self.cin, self.kh, self.kw, self.mb, self.deconv = cout_eff, cin, kh, kw, mb, bool(deconv)
        self.cout, self.bias = (cout_eff // 4 if deconv else cout_eff), None


def grid_sigs():
    out = []
    for cin, cout, (k, s, d, pad), (H, W), B in itertools.product(GRID_CIN, GRID_COUT, GRID_KERNELS, GRID_MAPS, GRID_B):
        mb = 1 if cout <= 16 else (4 if (cout >= 256 and cout % 64 == 0) else 2)  # PackedConv.mb
        out.append("%d,%d,%d,%d,%d,0|%d,%d,%d,%d,%d,%d,%d,%d,0" % (cout, cin, k, k, mb, H, W, B, s, s, d, d, pad))
    return out


def params(e):
    """ConvParams of the launch shape of Entry ``e``; the input map is the smallest a 'same'-style padding pl gives."""
    from codd_amd import _abi
    p = _abi.ConvParams()
    p.C0, p.B, p.Hout, p.Wout, p.terms, p.gate, p.dil2 = e.cin, e.B, e.H, e.W, e.terms, e.gate, e.dil2
    p.Cout, p.store_mode = (e.cout_eff // 4, 1) if e.deconv else (e.cout_eff, 0)
    p.kh, p.kw, p.sy, p.sx, p.pad_t, p.pad_l, p.dil_y, p.dil_x = e.kh, e.kw, e.sy, e.sx, e.pl, e.pl, e.dy, e.dx
    khe = e.kh // 2 if e.dil2 else e.kh
    p.Hin = max(1, (e.H - 1) * e.sy + (khe - 1) * e.dy + 1 - 2 * e.pl)
    p.Win = max(1, (e.W - 1) * e.sx + (e.kw - 1) * e.dx + 1 - 2 * e.pl)
    return p


def accepted(lib, p, pc, e):
    from codd_amd import ops
    return [c for c in ops._bf16_candidates(pc, e.H, e.W, e.B, e.kh * e.kw, e.terms) if ops._cfg_ok(lib, p, c)]


def plan_fp32(lib, e):
    from codd_amd import ops
    pc, p = Layer(e.cout_eff, e.cin, e.kh, e.kw, e.mb, e.deconv), params(e)
    pick = ops._conv_cfg(pc, e.H, e.W, e.B, e.sy, e.sx, e.dy, e.dx, e.pl)
    seen = []

    def recorder(lib, p, pc, cands, apply, desc):
        seen.append((list(cands), desc))
        return cands[0], 0.0

    real, ops._time_cfgs = ops._time_cfgs, recorder
    try:
        ops._autotune(lib, p, pc, tuple(pick) + (pc.mb, 0))
    finally:
        ops._time_cfgs = real
    return dict(pick=pick, tuned=seen)


def plan_split(lib, e):
    from codd_amd import ops
    pc, p = Layer(e.cout_eff, e.cin, e.kh, e.kw, e.mb, e.deconv), params(e)
    cands = accepted(lib, p, pc, e)
    return dict(cands=cands, small=ops._small_footprint(cands) if cands else [],
                dims_first=ops._split_dims(p, cands[:1]), dims_all=ops._split_dims(p, cands),
                fp32=ops._conv_cfg(pc, e.H, e.W, e.B, e.sy, e.sx, e.dy, e.dx, e.pl))


def plan_gate(lib, e):
    from codd_amd import ops
    pc, p = Layer(e.cout_eff, e.cin, e.kh, e.kw, 1, 0), params(e)
    cands = accepted(lib, p, pc, e)
    return dict(cands=ops._small_footprint(cands) if e.gate == 1 and cands else cands)


def plan(lib, sig):
    e = parse_sig(sig)
    return plan_gate(lib, e) if e.gate else plan_split(lib, e) if e.terms else plan_fp32(lib, e)


def _run_db(sigs):
    from codd_amd import _abi
    lib = _abi.load()
    return {"db/" + s: digest(plan(lib, s)) for s in sigs}


def _run_grid(sigs):
    from codd_amd import _abi
    lib = _abi.load()
    return {"grid/" + s: digest(dict(fp32=plan(lib, s), b3=plan(lib, "b3|" + s))) for s in sigs}


def _run_rows():
    from codd_amd import ops
    return {"split_rows/1..300": digest([ops._split_rows(H) for H in range(1, 301)])}


def groups():
    sigs = list(json.load(open(DB)))
    kinds = {"fp32": [], "split": [], "gate": []}
    for s in sigs:
        kinds["gate" if s[:1] == "g" else "split" if s[:1] == "b" else "fp32"].append(s)
    out = [("db_" + k, ["db/" + s for s in v], (lambda v=v: _run_db(v))) for k, v in kinds.items()]
    grid = grid_sigs()
    out.append(("grid", ["grid/" + s for s in grid], lambda: _run_grid(grid)))
    out.append(("split_rows", ["split_rows/1..300"], _run_rows))
    return out
