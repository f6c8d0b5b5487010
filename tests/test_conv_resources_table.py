"""profiles/conv_fp32_vec_epilogue_resources.txt -- the compile-time resources of every instantiation of the exact-fp32
convolution kernels, parent / new -- is held to what its change promised: no instantiation with scratch, a VGPR spill or
fewer waves per SIMD than its parent, every instantiation of the lists in conv_kernel.h / conv_quad_kernel.h present.  This
guards conv_min_blocks (conv_kernel.h), a launch bound whose effect depends on the compiler's register allocator: whoever
regenerates the table with another compiler sees a spill under the bound here, not on the GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = re.compile(r"^(conv_(?:mfma|quad|quad_multi)_kernel<[\d,]+>)\s+(\d+)/(\d+)\s+(\d+)/(\d+)\s+(\d+)/(\d+)\s+(\d+)/(\d+)\s+(\d+)/(\d+)\s*$")


def _rows():
    with open(os.path.join(ROOT, "profiles", "conv_fp32_vec_epilogue_resources.txt")) as f:
        return {m.group(1): tuple(int(v) for v in m.groups()[1:]) for m in map(ROW.match, f) if m}


def _listed():
    """Every X(...) of the instantiation lists, expanded from the headers' macros."""
    src = "".join(open(os.path.join(ROOT, "codd_amd", "csrc", h)).read() for h in ("conv_kernel.h", "conv_quad_kernel.h"))
    names = set()
    for npb, mb in re.findall(r"CONV_REGS_NW4\(X, (\d), (\d)\)", src):
        names |= {"conv_mfma_kernel<4,%s,%s,%d,%d>" % (npb, mb, w, i) for (w, i) in ((4, 4), (4, 8), (12, 4), (12, 8), (16, 8))}
    for nw, mb in re.findall(r"CONV_REGS_NWX\(X, (\d), (\d)\)", src):
        names |= {"conv_mfma_kernel<%s,1,%s,%d,4>" % (nw, mb, w) for w in (8, 16)}
    for line in re.findall(r"#define CONVQ_GROUP_\w\(X\)(.*)", src):
        names |= {"conv_quad_kernel<%s>" % ",".join(a.split(", ")) for a in re.findall(r"X\(([\d, ]+)\)", line)}
    for line in re.findall(r"#define CONVQ_MULTI\(X\)(.*)", src):
        names |= {"conv_quad_multi_kernel<%s>" % ",".join(a.split(", ")) for a in re.findall(r"X\(([\d, ]+)\)", line)}
    return names


def test_table_names_every_instantiation():
    rows, listed = _rows(), _listed()
    assert len(listed) == 81 and set(rows) == listed, (sorted(listed - set(rows))[:4], sorted(set(rows) - listed)[:4])


def test_no_instantiation_lost_occupancy_or_spills():
    bad = [k for k, (vp, vn, sp, sn, op, on, scp, scn, vsp, vsn) in _rows().items() if on < op or scn or vsn]
    assert not bad, bad


def test_the_bounded_instantiation_fits_its_bound():
    vp, vn, sp, sn, op, on, scp, scn, vsp, vsn = _rows()["conv_mfma_kernel<4,2,2,4,8>"]
    assert (on, scn, vsn) == (4, 0, 0) and vn <= 128
