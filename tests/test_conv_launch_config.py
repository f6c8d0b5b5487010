"""Stored conv launch configurations (codd_amd.ops.decode_cfg): every form the tuner, the tests and the shipped tune db
store decodes to the ConvParams fields the launch code writes, and every split-bf16 entry of the shipped db is one the
library accepts for the layer its signature describes (codd_conv2d_check: a dry run, no device)."""
import ctypes as C
import json
import os

import pytest

from codd_amd import _abi, ops

DB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "codd_amd", "tuned", "mi355x.json")
FIELDS = ("npb", "nw", "ck", "mb", "layout", "pgw", "cgw", "ksplit", "terms")


class _Packs:
    """Stands in for a PackedConv: records which packed-weight variant a configuration selects."""

    def __init__(self, mb):
        self.mb, self.asked = mb, []

    def packed(self, ck, mb=None, layout=0):
        self.asked.append((ck, mb, layout))
        return self

    def data_ptr(self):
        return 4096


# (stored configuration, PackedConv.mb, terms of the launch) -> ConvParams fields after ops._set_cfg, packed variant
# (ck, mb, layout); the fields of the other family keep their earlier values (pgw / cgw / ksplit = 5 / 6 / 7 here)
TABLE = [
    ((1, 4, 16), 2, 0, dict(npb=1, nw=4, ck=16, mb=2, layout=0, pgw=5, cgw=6, ksplit=7, terms=0), (16, 2, 0)),
    ((1, 9, 32, 4), 2, 0, dict(npb=1, nw=9, ck=32, mb=4, layout=0, pgw=5, cgw=6, ksplit=7, terms=0), (32, 4, 0)),
    ((2, 4, 16, 1, 1), 2, 3, dict(npb=2, nw=4, ck=16, mb=1, layout=1, pgw=5, cgw=6, ksplit=7, terms=0), (16, 1, 1)),
    ((2, 8, 16, 4, 2, 4, 1), 2, 3, dict(npb=2, nw=8, ck=16, mb=4, layout=2, pgw=4, cgw=1, ksplit=1, terms=3), (16, 4, 23)),
    ((1, 9, 16, 4, 2, 2, 2, 3), 1, 3, dict(npb=1, nw=9, ck=16, mb=4, layout=2, pgw=2, cgw=2, ksplit=1, terms=3), (16, 4, 23)),
    ((1, 10, 16, 4, 2, 2, 2, 48, 2), 4, 48, dict(npb=1, nw=10, ck=16, mb=4, layout=2, pgw=2, cgw=2, ksplit=2, terms=48),
     (16, 4, 68)),
]


@pytest.mark.parametrize("cfg,mb,terms,want,pack", TABLE)
def test_stored_forms_give_the_launch_fields(cfg, mb, terms, want, pack):
    p = _abi.ConvParams()
    p.pgw, p.cgw, p.ksplit, p.terms = 5, 6, 7, terms
    pc = _Packs(mb)
    ops._set_cfg(p, cfg, pc)
    assert {k: getattr(p, k) for k in FIELDS} == want
    assert pc.asked == [pack] and p.wpacked == 4096
    f = ops.decode_cfg(cfg, mb, terms)
    assert (f.npb, f.nw, f.ck, f.mb, f.layout) == tuple(want[k] for k in ("npb", "nw", "ck", "mb", "layout"))
    if len(cfg) != 7:  # (a stored split configuration names its terms: pc.tuned / TUNE_DB never hold seven fields)
        assert ops.PackedConv._pack_key(pc, cfg) == (pack[1], pack[0], pack[2])


def test_malformed_configurations_are_refused():
    for bad in [(1, 4), (1, 4, 16, 2, 0, 0), (1, 4, 16, 2, 3), (2, 8, 16, 4, 2, 4), (1, 9, 16, 4, 2, 2, 2, 3, 1, 0)]:
        with pytest.raises(ValueError):
            ops.decode_cfg(bad, 2, 3)


def _layer(sig):
    """ConvParams of the layer a tune-db signature describes (only what codd_conv2d_check reads); the signature formats
    are stated once, in the comment above ops._plain_key."""
    p = _abi.ConvParams()
    head, w, shape = sig.split("|")[:3]
    if head.startswith("g"):  # gate epilogue: "g<gate>,b<terms>|cout,cin,kh,kw|H,W,B,pad,dil,dil2"
        gate, terms = (int(v[1:]) for v in head.split(","))
        cout, cin, kh, kw = map(int, w.split(","))
        H, W, B, pad, dil, dil2 = map(int, shape.split(","))
        p.gate, p.dil2, p.terms = gate, dil2, terms
        p.C0, p.B, p.Cout, p.Hout, p.Wout, p.Hin, p.Win = cin, B, cout, H, W, H, W
        p.kh, p.kw, p.sy, p.sx, p.pad_t, p.pad_l, p.dil_y, p.dil_x = kh, kw, 1, 1, pad, pad, dil, dil
        return p
    # "b<terms>|cout_eff,cin,kh,kw,mb,deconv|Hout,Wout,B,sy,sx,dy,dx,pl,two inputs[|split][|co]"
    p.terms = int(head[1:])
    cout_eff, cin, kh, kw, _, deconv = map(int, w.split(","))
    Hout, Wout, B, sy, sx, dy, dx, pl, _ = map(int, shape.split(","))
    p.C0, p.B, p.Hout, p.Wout = cin, B, Hout, Wout
    p.Cout, p.store_mode = (cout_eff // 4, 1) if deconv else (cout_eff, 0)
    p.kh, p.kw, p.sy, p.sx, p.pad_t, p.pad_l, p.dil_y, p.dil_x = kh, kw, sy, sx, pl, pl, dy, dx
    return p


def test_shipped_tune_db_decodes_and_its_split_entries_are_accepted():
    db = json.load(open(DB))
    lib = _abi.load()
    n_split = 0
    for sig, cfg in db.items():
        sig_terms = int(sig.split("|")[0].split(",")[-1][1:]) if sig.split("|")[0][:1] in "bg" else 0
        f = ops.decode_cfg(cfg, 1, sig_terms)
        if f.layout != 2:
            assert len(cfg) in (3, 4, 5), (sig, cfg)
            continue
        n_split += 1
        p = _layer(sig)
        assert f.terms == p.terms and p.terms, (sig, cfg)
        ops._set_cfg(p, cfg)
        assert lib.codd_conv2d_check(C.byref(p)) == 0, (sig, cfg)
    assert n_split > 200, n_split


def test_library_instantiations_are_the_headers_and_tiles_match():
    """codd_conv2d_bf16_instantiations (what ops._B_INST reads) is the CONVB_ALL expansion of conv_bf16_kernel.h, and
    ops._B_TILES lists tiles for exactly the pixel-unit counts (pgw * A) of those instantiations."""
    from convb_epilogue_cases import header_convb_all
    lib = _abi.load()
    n = lib.codd_conv2d_bf16_instantiations(None, 0)
    flat = (C.c_int * (5 * n))()
    assert lib.codd_conv2d_bf16_instantiations(flat, n) == n
    got = [tuple(flat[5 * i:5 * i + 5]) for i in range(n)]
    assert got == header_convb_all() and len(set(got)) == n > 0
    assert list(ops._B_INST) == got
    short = (C.c_int * 10)(*([-7] * 10))  # cap: only whole quintuples below it are written
    assert lib.codd_conv2d_bf16_instantiations(short, 1) == n and list(short) == list(got[0]) + [-7] * 5
    assert set(ops._B_TILES) == {pgw * a for (pgw, _, a, _, _) in got}
    for units, tiles in ops._B_TILES.items():  # the dispatch runs a tile of th * xb units on A = ceil(th * xb / pgw)
        grids = {(pgw, a) for (pgw, _, a, _, _) in got if pgw * a == units}
        assert tiles and all(xb in (1, 2) and any(-(-th * xb // pgw) == a for (pgw, a) in grids) for (th, xb) in tiles), (units, tiles)
