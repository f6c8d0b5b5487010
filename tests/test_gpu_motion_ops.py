"""GPU parity of the Motion / RAFT3D / Fusion kernels against the CPU oracle (fp32)."""
import os
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def rnd(*s, seed=0):
    g = torch.Generator().manual_seed(seed + sum(s))
    return torch.randn(*s, generator=g)


def rel(a, b):
    return (a - b).abs().max().item() / max(1e-6, b.abs().max().item())


def test_instnorm():
    from codd_amd import ops
    x, r = rnd(2, 64, 36, 60) * 3 + 1, rnd(2, 64, 36, 60, seed=1)
    ref = F.relu(F.instance_norm(x) + r)
    got = ops.instnorm(x.to(DEV), relu=True, res=r.to(DEV)).cpu()
    assert (got - ref).abs().max().item() < 1e-4


def test_allpairs_and_lookup():
    from codd_amd import ops
    from oracle import motion as om
    h, w = 24, 40
    f1, f2 = rnd(1, 128, h, w), rnd(1, 128, h, w, seed=1)
    pyr_ref = om.corr_pyramid(f1, f2)
    pyr = ops.allpairs_corr(f1.to(DEV), f2.to(DEV))
    for a, b in zip(pyr, pyr_ref):
        assert rel(a.cpu().view(-1), b.reshape(-1)) < 1e-4
    g = torch.Generator().manual_seed(5)
    coords = torch.rand(1, h, w, 3, generator=g) * torch.tensor([w + 8.0, h + 8.0, 1.0]) - 4.0
    coords[0, 0, 0] = torch.tensor([3.0, 2.0, 0.0])  # exact integer position
    coords[0, 0, 1] = torch.tensor([-50.0, 1e6, 0.0])  # far outside
    ref = om.corr_lookup(pyr_ref, coords[..., :2].permute(0, 3, 1, 2).contiguous())
    got = ops.corr_lookup(pyr, coords.to(DEV), h, w).cpu()
    assert got.shape == ref.shape == (1, 196, h, w)
    assert (got - ref).abs().max().item() < 1e-4 * max(1.0, ref.abs().max().item())


def _se3_field(B, h, w, scale=0.05, seed=0):
    from oracle import se3
    return se3.exp(rnd(B, h, w, 6, seed=seed) * scale)


def test_raft_geometry():
    from codd_amd import ops
    from oracle import motion as om, se3
    B, h, w = 1, 16, 32
    T = _se3_field(B, h, w)
    g = torch.Generator().manual_seed(3)
    d1 = torch.rand(B, h, w, generator=g) * 40 + 2
    d2 = torch.rand(B, h, w, generator=g) * 40 + 2
    K8 = [35.0, 36.0, 16.0, 8.0]
    Kt = torch.tensor([K8])
    xyz_ref = om.project(se3.act(T, om.inv_project(d1, Kt)), Kt)
    coords1, zp = xyz_ref[..., :2], xyz_ref[..., 2:]
    zinv = om.sample_bilinear((1.0 / d2)[:, None], coords1)
    y0, x0 = torch.meshgrid(torch.arange(h).float(), torch.arange(w).float(), indexing="ij")
    c0 = torch.stack([x0, y0], -1)[None]
    mi_ref = om.motion_info(coords1 - c0, se3.log(T), zinv.unsqueeze(-1) - zp)
    xyz, mi = ops.raft_geometry(T.to(DEV), d1.to(DEV), d2.to(DEV), K8)
    assert (xyz.cpu() - xyz_ref).abs().max().item() < 1e-3 * xyz_ref.abs().max().item()
    assert (mi.cpu() - mi_ref).abs().max().item() < 2e-4 * max(1.0, mi_ref.abs().max().item())


@pytest.mark.parametrize("h,w,radius", [(12, 20, 32), (20, 44, 6)])
def test_se3_gn_step(h, w, radius):
    from codd_amd import ops
    from oracle import motion as om, se3
    B = 1
    T = _se3_field(B, h, w, 0.03)
    g = torch.Generator().manual_seed(7)
    d1 = torch.rand(B, h, w, generator=g) * 30 + 3
    K8 = [40.0, 42.0, w / 2.0, h / 2.0]
    Kt = torch.tensor([K8])
    ae = rnd(B, 32, h, w, seed=2) * 4
    xyz = om.project(se3.act(T, om.inv_project(d1, Kt)), Kt)
    delta = rnd(B, 3, h, w, seed=3) * torch.tensor([1.0, 1.0, 0.01]).view(1, 3, 1, 1)
    weight = torch.sigmoid(rnd(B, 3, h, w, seed=4))
    target = (xyz.permute(0, 3, 1, 2) + delta).contiguous()
    pts = om.inv_project(d1, Kt).permute(0, 3, 1, 2).contiguous()
    Hm, bm = om.se3_build(T, ae / 8.0, pts, target, weight, Kt, radius=radius)
    T_ref = se3.compose(se3.exp(om.gn_solve(Hm, bm)), T)
    Tg = T.to(DEV).clone()
    ops.se3_gn_step(Tg, ae.to(DEV), xyz.to(DEV), delta.to(DEV), weight.to(DEV), d1.to(DEV), K8, radius=radius)
    err = (Tg.cpu() - T_ref).abs().max().item()
    step = (T_ref - T).abs().max().item()
    print("gn step size", step, "err", err)
    assert err < 2e-4 * max(1.0, T_ref.abs().max().item()) and err < 0.02 * step


def test_cvx_upsample():
    from codd_amd import ops
    from oracle import motion as om
    B, h, w = 1, 9, 70
    mask = rnd(B, 576, h, w) * 2
    T = _se3_field(B, h, w, 0.2)
    ref = om.upsample_se3(T, mask)
    got = ops.cvx_upsample(T.to(DEV), mask.to(DEV), 1).cpu()
    assert (got - ref).abs().max().item() < 1e-5
    wgt = rnd(B, 3, h, w, seed=1)
    ref = om.cvx_upsample(wgt.permute(0, 2, 3, 1), mask).permute(0, 3, 1, 2)
    got = ops.cvx_upsample(wgt.to(DEV), mask.to(DEV), 2).cpu()
    assert (got - ref).abs().max().item() < 1e-5
    # both with one pass over the mask (what RAFT3D.forward launches after the last update)
    To, wo = ops.cvx_upsample_se3_weight(T.to(DEV), wgt.to(DEV), mask.to(DEV))
    assert (To.cpu() - om.upsample_se3(T, mask)).abs().max().item() < 1e-5
    assert (wo.cpu() - ref).abs().max().item() < 1e-5


@pytest.mark.parametrize("ds,radius,C", [(1, 2.0, 6), (4, 4.0, 32)])
def test_splat(ds, radius, C):
    from codd_amd import ops
    from oracle import motion as om
    B, HT, WT = 1, 64, 96
    T = _se3_field(B, HT, WT, 0.02)
    g = torch.Generator().manual_seed(11)
    depth = torch.rand(B, HT, WT, generator=g) * 20 + 5
    depth[0, 10:14, 20:30] = 0.0  # culled points
    o = ds // 2 - 1 if ds > 1 else 0
    H, W = HT // ds, WT // ds
    K = [60.0 / ds, 62.0 / ds, WT / 2.0 / ds, HT / 2.0 / ds]
    feat = rnd(B, C, H, W, seed=2)
    Ts, ds_ = T[:, o::ds, o::ds], depth[:, o::ds, o::ds]
    ref, zref = om.splat(Ts, ds_, feat, torch.tensor([K]), radius)
    got, z = ops.splat(T.to(DEV), depth.to(DEV), feat.to(DEV), None, False, H, W, o, o, ds, K, radius)
    bad = ((got.cpu() - ref).abs().amax(1) > 1e-3).float().mean().item()
    badz = ((z.cpu() - zref).abs() > 1e-3).float().mean().item()
    print("splat mismatching pixels", bad, badz, "coverage", (zref > 0).float().mean().item())
    assert bad < 1e-4 and badz < 1e-4  # (measured on MI355X: 0 mismatching pixels)
    # with induced flow + disparity conversion
    if ds == 1:
        bf = 210.0
        got, dsp = ops.splat(T.to(DEV), depth.to(DEV), feat[:, :3].to(DEV), feat[:, 3:].to(DEV), True, H, W, 0, 0, 1, K,
                             radius, bf=bf)
        flow = om.induced_flow2d(T, depth, torch.tensor([K])).permute(0, 3, 1, 2)
        ref, zref = om.splat(T, depth, torch.cat([feat[:, :3], flow, feat[:, 3:]], 1), torch.tensor([K]), radius)
        dref = bf / (zref + 1e-5)
        dref = torch.where(dref > W, torch.zeros_like(dref), dref)
        assert ((got.cpu() - ref).abs().amax(1) > 1e-3).float().mean().item() < 1e-3
        assert ((dsp.cpu() - dref).abs() > 1e-3 * (1 + dref.abs())).float().mean().item() < 1e-3


def test_splat_pileup_keeps_the_eight_nearest_of_all_candidates():
    """Thousands of points driven onto three pixels (far beyond any fixed per-pixel capacity), many with EXACTLY
    equal depth: the exact-size candidate lists must give the oracle's top-8-by-(z, index) composite, bit-for-bit
    reproducibly across runs (the atomics' order must not matter)."""
    from codd_amd import ops
    from oracle import motion as om
    B, H, W, C = 1, 48, 64, 5
    K = [40.0, 42.0, 32.0, 24.0]
    Kt = torch.tensor([K])
    g = torch.Generator().manual_seed(5)
    depth = torch.rand(B, H, W, generator=g) * 10 + 3
    X0 = om.inv_project(depth, Kt).reshape(-1, 3)
    n = torch.arange(H * W)
    tgt = torch.tensor([[20.5, 10.5], [21.5, 10.5], [40.5, 30.5]])[n % 3]  # three target pixels (two adjacent)
    tz = torch.where(n % 4 == 0, torch.full((H * W,), 4.0), 4.0 + 0.001 * (n % 211).float())
    tu = tgt[:, 0] + 0.4 * torch.sin(n.float() * 0.37)
    tv = tgt[:, 1] + 0.4 * torch.cos(n.float() * 0.73)
    P = torch.stack([(tu - K[2]) * tz / K[0], (tv - K[3]) * tz / K[1], tz], -1)
    T = torch.zeros(B, H, W, 7)
    T[..., 6] = 1.0
    T[0].view(-1, 7)[:, :3] = P - X0  # pure translations: T * X0 = P
    feat = rnd(B, C, H, W, seed=2)
    ref, zref = om.splat(T, depth, feat, Kt, 2.0)
    outs = []
    for _ in range(3):
        got, z = ops.splat(T.to(DEV), depth.to(DEV), feat.to(DEV), None, False, H, W, 0, 0, 1, K, 2.0)
        outs.append((got.cpu(), z.cpu()))
    assert all(torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]) for o in outs[1:]), "run-to-run differences"
    assert (outs[0][0] - ref).abs().max().item() < 1e-4 and (outs[0][1] - zref).abs().max().item() < 1e-5
    assert (zref > 0).sum().item() <= 30  # everything really is piled onto a handful of pixels (~1000 points each)


def _model(iters=2):
    import codd_amd  # noqa: F401
    from codd_amd import configs, synth
    from codd_amd.registry import build_estimator
    est = build_estimator(configs.codd(iters=iters)).eval()
    synth.load_synthetic_weights(est, gain=1.4)
    sd = {k: v.clone() for k, v in est.state_dict().items()}
    return est.to(DEV), sd


def test_fnet_cnet_update_block():
    from oracle import motion as om
    est, sd = _model()
    r3 = est.motion.raft3d
    x = rnd(1, 3, 128, 192)
    ref = om.basic_encoder(sd, "motion.raft3d.fnet", x)
    got = r3.fnet(x.to(DEV)).cpu()
    assert rel(got, ref) < 2e-4, rel(got, ref)
    ref = om.hrnet_cnet(sd, "motion.raft3d.cnet", x)
    got = r3.context(x.to(DEV)).cpu()
    assert got.shape == ref.shape == (1, 512, 16, 24)
    assert rel(got, ref) < 2e-4, rel(got, ref)
    net, inp, corr, minfo = rnd(1, 128, 16, 24), rnd(1, 384, 16, 24, seed=1), rnd(1, 196, 16, 24, seed=2), \
        rnd(1, 9, 16, 24, seed=3)
    refs = om.update_block(sd, "motion.raft3d.update_block", net, inp, corr, minfo)
    gots = r3.update_block.run(net.to(DEV), inp.to(DEV), corr.to(DEV), minfo.to(DEV), True)[:5]
    for name, a, b in zip(("net", "mask", "ae", "delta", "weight"), gots, refs):
        assert rel(a.cpu(), b) < 2e-4, (name, rel(a.cpu(), b))


def test_fusion_query():
    from oracle import fusion as ofu
    est, sd = _model()
    H, W = 64, 128
    g = torch.Generator().manual_seed(0)
    R = lambda *s: torch.randn(*s, generator=g)
    pred = (R(1, 1, H, W) * 5 + 20).abs()
    pw = (R(1, 1, H, W) * 5 + 20).abs()
    pw[:, :, 10:20, 30:50] = 0
    out = dict(left_feat=R(1, 24, H // 4, W // 4), right_feat=R(1, 24, H // 4, W // 4), pred_disp=pred,
               left_img=R(1, 3, H, W))
    mem = [R(1, 3, H, W), R(1, 32, H // 4, W // 4), torch.rand(1, 3, H, W, generator=g), pw, R(1, 3, H, W)]
    o_ref = dict(out)
    ofu.memory_query(sd, o_ref, dict(memory=mem))
    o_gpu = {k: v.to(DEV) for k, v in out.items()}
    est.fusion.memory_query(o_gpu, dict(memory=[m.to(DEV) for m in mem]))
    for k in ("left_feat", "fusion_weights", "reset_weights", "pred_disp"):
        assert rel(o_gpu[k].cpu(), o_ref[k]) < 2e-4, (k, rel(o_gpu[k].cpu(), o_ref[k]))


@pytest.mark.parametrize("patch,ds", [(5, 4), (3, 2)])
def test_fusion_non_default_geometry(patch, ds):
    """Fusion with corr_cfg.patch_size != 3 / ds_scale != 4 (reference fusion.py:55-72 is generic): HIP vs the oracle,
    and for patch_size = 5 vs the REFERENCE's own output (tests/golden: fusion_p5_*)."""
    import numpy as np
    from codd_amd.registry import MODELS
    from oracle import fusion as ofu
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import cases
    fus = MODELS.build(dict(type="Fusion", in_channels=24, fusion_channel=32, corr_cfg=dict(type="px2patch", patch_size=patch),
                            ds_scale=ds)).eval()
    if patch == 5:
        sd = cases.fusion_p5_state_dict()
    else:
        g = torch.Generator().manual_seed(3)
        sd = {"fusion." + k: (cases.state_dict()["fusion." + k] if cases.state_dict()["fusion." + k].shape == v.shape
                              else torch.randn(v.shape, generator=g) * (1.4 / v[0].numel() ** 0.5))
              for k, v in fus.state_dict().items()}
    fus.load_state_dict({k[len("fusion."):]: v for k, v in sd.items()})
    fus = fus.to(DEV)
    o, st = cases.fusion_case()
    if ds != 4:  # the stereo / memory features live at 1/ds resolution
        H, W = o["pred_disp"].shape[-2:]
        R = cases._gen(7)
        o["left_feat"], o["right_feat"] = R(1, 24, H // ds, W // ds), R(1, 24, H // ds, W // ds)
        st["memory"][1] = R(1, 32, H // ds, W // ds)
    o_ref = dict(o)
    with torch.no_grad():
        ofu.memory_query(sd, o_ref, dict(memory=list(st["memory"])), patch_size=patch, ds=ds)
        o_gpu = {k: v.to(DEV) for k, v in o.items()}
        fus.memory_query(o_gpu, dict(memory=[m.to(DEV) for m in st["memory"]]))
    for k in ("fusion_weights", "reset_weights", "pred_disp"):
        assert rel(o_gpu[k].cpu(), o_ref[k]) < 2e-4, (k, rel(o_gpu[k].cpu(), o_ref[k]))
    if patch == 5:
        G = np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_outputs.npz"))
        for k in ("fusion_weights", "reset_weights", "pred_disp"):
            ref = torch.from_numpy(G[f"fusion_p5_{k}"])
            assert rel(o_gpu[k].cpu(), ref) < 2e-4, (k, rel(o_gpu[k].cpu(), ref))


@pytest.mark.parametrize("iters", [2])
def test_full_codd_sequence(iters):
    from codd_amd import synth
    from oracle import codd as oc
    est, sd = _model(iters)
    H, W, MF = 128, 256, 3
    img, r_img, _ = synth.stereo_sequence(H, W, MF)
    metas = synth.default_metas(H, W, intrinsics=(280.0, 280.0, 128.0, 64.0))
    ref = oc.inference(sd, img, r_img, metas, iters=iters)
    got = est(img=[img.to(DEV)], img_metas=metas, return_loss=False, r_img=[r_img.to(DEV)], evaluate=False)[0].cpu()
    assert got.shape == ref.shape == (1, MF, H, W)
    for f in range(MF):
        epe = (got[:, f] - ref[:, f]).abs().mean().item()
        print(f"frame {f}: EPE delta {epe:.3e}  max {(got[:, f] - ref[:, f]).abs().max().item():.3e}")
        assert epe < 1e-3


def test_disp_metrics_kernel_matches_torch_reference():
    from codd_amd import metrics
    H, W, h, w = 64, 96, 60, 90
    meta = dict(disp_range=(1, 210))
    sm_t, sm_d = metrics.SequenceMetrics(meta, torch.device("cpu")), metrics.SequenceMetrics(meta, torch.device(DEV))
    for f in range(3):
        gt = (rnd(1, 1, H, W, seed=f) * 40 + 60).clamp(0, 250)
        gt[0, 0, 5:9, 7:30] = 0.0  # invalid
        pred = gt + rnd(1, 1, H, W, seed=10 + f) * 3
        sm_t.update(pred[:, :, :h, :w], gt[:, :, :h, :w])
        sm_d.update_disparity_device(pred.to(DEV), gt.to(DEV), (h, w))
    rt, rd = sm_t.row(), sm_d.row().cpu()
    assert abs(rt[0].item() - rd[0].item()) < 1e-6 and abs(rt[1].item() - rd[1].item()) < 1e-9


@pytest.mark.parametrize("H,W,intr", [(128, 384, (240.0, 240.0, 190.0, 62.0))])
def test_full_codd_kitti_aspect_matches_oracle(H, W, intr):
    """BASELINE config 4 aspect ratio (1242x375 -> 1280x384) scaled down, iters=4, through hipGraph replay.

    With random-init weights the estimated motion is wild (|t| ~ 0.4 per frame), many splatted points
    pass close to the camera and the warped disparity bf/z takes values of several hundred px: the
    discontinuous selections of the path (nearest-z point, `disp_warp > W -> 0`, `pred_warp > 0`
    masks; SURVEY.md section 7 'hard parts') then flip for a handful of pixels under 1e-6 input
    differences and each flip costs hundreds of px.  The test therefore bounds the FRACTION of
    flipped pixels and the EPE over the others (the north-star 1e-3 bound), and requires graph
    replay to be bit-identical to eager execution."""
    from codd_amd import synth
    from codd_amd.runtime import FrameRunner
    from oracle import codd as oc
    est, sd = _model(4)
    MF = 3
    img, r_img, _ = synth.stereo_sequence(H, W, MF)
    metas = synth.default_metas(H, W, intrinsics=intr)
    ref = oc.inference(sd, img, r_img, metas, iters=4)
    rg, re = FrameRunner(est, metas[0], use_graph=True), FrameRunner(est, metas[0], use_graph=False)
    for f in range(MF):
        l, r = img[:, f].to(DEV).contiguous(), r_img[:, f].to(DEV).contiguous()
        d = rg.step(l, r).clone()
        assert torch.equal(d, re.step(l, r)), "graph replay differs from eager execution"
        diff = (d.cpu()[:, 0] - ref[:, f]).abs()
        flipped = diff > 0.25
        epe_rest = diff[~flipped].mean().item()
        print(f"frame {f} (graph={rg.graph is not None}): flipped {flipped.float().mean().item():.2e}, "
              f"EPE delta elsewhere {epe_rest:.3e}, raw EPE delta {diff.mean().item():.3e}")
        assert flipped.float().mean().item() < 5e-4 and epe_rest < 1e-3  # (measured: no flipped pixel)


@pytest.mark.parametrize("H,W,intr", [(384, 1280, (721.54, 721.54, 621.0, 187.5)), (512, 640, (320.0, 320.0, 320.0, 240.0))])
def test_full_codd_runs_at_baseline_shapes(H, W, intr):
    """BASELINE configs 3 / 4 padded shapes, iters = 16, heuristic (un-tuned) launch configurations: five frames by graph
    replay must reproduce the eager launch schedule frame for frame (same kernels, same arguments: the captured graph
    may not drop, reorder or alias anything at these non-square shapes).  Parity against the oracle at these shapes is
    tests/test_gpu_headline_parity.py."""
    from codd_amd import synth
    from codd_amd.runtime import FrameRunner
    est, _ = _model(16)
    img, r_img, _ = synth.stereo_sequence(H, W, 3)
    metas = synth.default_metas(H, W, intrinsics=intr)
    rg, re = FrameRunner(est, metas[0], use_graph=True), FrameRunner(est, metas[0], use_graph=False)
    for f in range(5):
        l, r = img[:, f % 3].to(DEV).contiguous(), r_img[:, f % 3].to(DEV).contiguous()
        d, e = rg.step(l, r).clone(), re.step(l, r)
        assert d.shape == (1, 1, H, W) and torch.isfinite(d).all()
        assert (d - e).abs().max().item() < 1e-4, (f, (d - e).abs().max().item())
    assert rg.graph is not None


def test_tepe_metrics_kernel_matches_torch_reference():
    from codd_amd import metrics
    H, W, h, w = 64, 96, 60, 90
    meta = dict(disp_range=(1, 210))
    sm_t, sm_d = metrics.SequenceMetrics(meta, torch.device("cpu")), metrics.SequenceMetrics(meta, torch.device(DEV))
    prev = None
    for f in range(4):
        gt = (rnd(1, 1, H, W, seed=f) * 40 + 60).clamp(0, 250)
        gt[0, 0, 5:9, 7:30] = 0.0
        pred = gt + rnd(1, 1, H, W, seed=10 + f) * 3
        flow = rnd(1, 2, H, W, seed=20 + f) * 2.5
        sm_t.update(pred[:, :, :h, :w], gt[:, :, :h, :w], flow[:, :, :h, :w])
        pd, gd, fd = pred.to(DEV), gt.to(DEV), flow.to(DEV)
        sm_d.update_disparity_device(pd, gd, (h, w))
        if prev is not None:
            sm_d.update_temporal_device(pd, gd, prev[0], prev[1], prev[2], (h, w))
        prev = (pd, gd, fd)
    rt, rd = sm_t.row(), sm_d.row().cpu()
    for i in range(7):
        assert abs(rt[i].item() - rd[i].item()) < 1e-5 * max(1.0, abs(rt[i].item())), (metrics.COLUMNS[i], rt[i], rd[i])


def test_sceneflow_metrics_kernel_matches_torch_restatement():
    """HIP scene-flow accumulators vs codd_amd.metrics.scene_flow_sums (itself pinned to the reference's calc_metric by
    tests/test_oracle_golden.py), on padded maps with a crop, zero predictions, invalid GT and occlusions."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import cases
    from codd_amd import metrics
    sc = cases.sceneflow_case()
    h, w = sc["h"], sc["w"]
    for with_occ in (False, True):
        st, sd = metrics.SequenceMetrics(sc["meta"], torch.device("cpu")), metrics.SequenceMetrics(sc["meta"], torch.device(DEV))
        for f in range(1, sc["pred"].shape[1]):
            dc = sc["dchange"][:, f if with_occ else f - 1]
            occ = sc["occ"][:, f - 1] if with_occ else None
            crop = lambda t_: t_[..., :h, :w]
            st.update_scene_flow(sc["Ts"][:, f, :h, :w], crop(sc["pred"][:, f - 1]), crop(sc["gt"][:, f - 1]),
                                 crop(sc["flow"][:, f - 1]), crop(dc), None if occ is None else crop(occ))
            sd.update_scene_flow_device(sc["Ts"][:, f].to(DEV), sc["pred"][:, f - 1].to(DEV), sc["gt"][:, f - 1].to(DEV),
                                        sc["flow"][:, f - 1].contiguous().to(DEV), dc.to(DEV),
                                        None if occ is None else occ.to(DEV), (h, w))
        a, b = st.row()[7:], sd.row()[7:].cpu()
        assert a[0].item() == b[0].item() and a[0].item() > 1000
        for i in range(1, 5):
            assert abs(a[i].item() - b[i].item()) <= 1e-4 * max(1.0, abs(a[i].item())) + (2.0 if i >= 3 else 0.0), (i, a[i], b[i])
    with pytest.raises(ValueError):  # unpadded ground truth is refused instead of being read out of bounds
        sd.update_scene_flow_device(sc["Ts"][:, 1].to(DEV), sc["pred"][:, 0].to(DEV), sc["gt"][:, 0, :, :h, :w].to(DEV),
                                    sc["flow"][:, 0].contiguous().to(DEV), sc["dchange"][:, 0].to(DEV), None, (h, w))


def test_motion_outputs_follow_the_reference_dict_contract():
    """reference raft3d.py:267-274: motion writes outputs['Ts'], ['flow2d_est_induced'] and ['weight']; the induced
    flow equals the oracle's induced_flow2d of the up-sampled field."""
    from codd_amd import synth
    from oracle import motion as om
    est, _ = _model(2)
    H, W = 128, 256
    img, r_img, _ = synth.stereo_sequence(H, W, 2)
    metas = synth.default_metas(H, W, intrinsics=(280.0, 280.0, 128.0, 64.0))[0]
    state = {}
    for f in range(2):
        out = est.consistent_online_depth_estimation(img[:, f].to(DEV).contiguous(), r_img[:, f].to(DEV).contiguous(), metas, state)
        if f == 0:
            depth_prev = (210.0 / (out["pred_disp"][:, 0] + 1e-5)).clamp(0, 210.0).cpu()
    assert out["Ts"].shape == (1, H, W, 7) and out["weight"].shape == (1, 3, H, W)
    fl = out["flow2d_est_induced"]
    assert fl.shape == (1, H, W, 3)
    ref = om.induced_flow2d(out["Ts"].cpu(), depth_prev, torch.tensor([[280.0, 280.0, 128.0, 64.0]]))
    assert (fl.cpu() - ref).abs().max().item() < 1e-3 * max(1.0, ref.abs().max().item())


def test_preprocess_matches_numpy_restatement():
    import numpy as np
    from codd_amd import ops
    g = np.random.RandomState(0)
    img = g.randint(0, 256, size=(100, 150, 3), dtype=np.uint8)  # BGR HWC like cv2.imread
    out = ops.preprocess(torch.from_numpy(img).to(DEV), bgr=True).cpu().numpy()[0]
    rgb = img[:, :, ::-1].astype(np.float32)
    norm = (rgb - np.array(ops.IMAGENET_MEAN, np.float32)) / np.array(ops.IMAGENET_STD, np.float32)
    ref = np.pad(norm, ((0, 28), (0, 42), (0, 0)), mode="reflect").transpose(2, 0, 1)  # -> 128 x 192
    assert out.shape == ref.shape == (3, 128, 192)
    assert np.abs(out - ref).max() < 1e-5


def test_eval_harness_on_device_metrics_match_torch_restatement(tmp_path):
    """apis.single_gpu_inference(evaluate=True) on two synthetic videos: the HIP metric kernels inside
    estimator.inference must give the same row as the torch restatement applied to the disparities
    returned by evaluate=False; a checkpoint round trip through apis.load_checkpoint must not change them."""
    from codd_amd import apis, configs, metrics, synth
    from codd_amd.registry import build_estimator
    H, W, MF = 128, 256, 3
    est = build_estimator(configs.codd(iters=2)).to(DEV).eval()
    synth.load_synthetic_weights(est, gain=1.4)
    videos, rows_ref = [], []
    for v in range(2):
        left, right, disp = synth.stereo_sequence(H, W, MF, 32.0, flow=(0.75 + v, 0.25))
        metas = synth.default_metas(H, W, img_shape=(120, 250))
        metas[0][0].update(filename="vid%d" % v, ori_filename="vid%d.png" % v, disp_range=(1, 210))
        flow = rnd(1, MF, 2, H, W, seed=50 + v) * 2
        videos.append(dict(img=[left.to(DEV)], r_img=[right.to(DEV)], img_metas=metas,
                           gt_disp=[(disp + v).to(DEV)], gt_flow=[flow.to(DEV)]))
    torch.save(dict(state_dict=est.state_dict()), str(tmp_path / "w.pth"))
    apis.load_checkpoint(est, str(tmp_path / "w.pth"), strict=True)
    summary = apis.single_gpu_inference(est, videos, out_dir=str(tmp_path), evaluate=True)
    for d in videos:
        pred = est(img=d["img"], r_img=d["r_img"], img_metas=d["img_metas"], return_loss=False, evaluate=False)[0]
        sm = metrics.SequenceMetrics(d["img_metas"][0][0], torch.device(DEV))
        for f in range(MF):
            sm.update(pred[:, f:f + 1], d["gt_disp"][0][:, f, :, :120, :250], d["gt_flow"][0][:, f, :, :120, :250])
        rows_ref.append(sm.row().cpu())
    ref = metrics.reduce_rows(rows_ref, torch.device("cpu"))
    for k in metrics.COLUMNS[:7]:
        assert abs(summary[k][0] - ref[k][0]) < 1e-5 * max(1.0, abs(ref[k][0])), (k, summary[k], ref[k])
    assert (tmp_path / "stats.csv").exists()


def test_inference_with_kitti_style_ground_truth_and_derived_disp_change():
    """estimator.inference(evaluate=True) with gt_disp2 / gt_disp_occ (and, on the full model, gt_flow_occ without
    gt_disp_change: the disparity change is derived as utils/misc.py:39-59 does): the on-device rows must equal the torch
    restatement driven with the same inputs (which is pinned to the reference in tests/test_oracle_golden.py)."""
    from codd_amd import configs, metrics as M, synth
    from codd_amd.registry import build_estimator
    H, W, MF, h, w = 128, 256, 3, 120, 250
    est = build_estimator(configs.codd(iters=2)).to(DEV).eval()
    synth.load_synthetic_weights(est, gain=1.4)
    left, right, disp = synth.stereo_sequence(H, W, MF, 32.0)
    metas = synth.default_metas(H, W, img_shape=(h, w))
    metas[0][0].update(disp_range=(1, 210))
    gt = disp.clone()
    gt[:, 1] = 0.0  # no ground truth on frame 1
    gt2 = (disp + 0.5 * rnd(1, MF, 1, H, W, seed=3)).clamp(min=0)
    occ = (rnd(1, MF, 1, H, W, seed=4) > 1.0).float()
    flow = rnd(1, MF, 2, H, W, seed=5) * 2
    focc = (rnd(1, MF, 1, H, W, seed=6) > 1.2).float()
    d = lambda t: [t.to(DEV)]
    kw = dict(gt_disp=d(gt), gt_flow=d(flow), gt_disp2=d(gt2), gt_disp_occ=d(occ))
    row = est(img=d(left), r_img=d(right), img_metas=metas, return_loss=False, evaluate=True, **kw)[0]
    pred = est(img=d(left), r_img=d(right), img_metas=metas, return_loss=False, evaluate=False)[0].cpu()
    sm = M.SequenceMetrics(metas[0][0], torch.device("cpu"))
    c = lambda t, f: t[:, f, :, :h, :w]
    for f in range(MF):
        sm.update(pred[:, f:f + 1], c(gt, f), c(flow, f), seg=c(occ, f) <= 0, gt_disp2=c(gt2, f))
    ref = sm.row()
    for i, k in enumerate(M.COLUMNS[:7]):
        got = float(row[k][0])
        assert abs(got - ref[i].item()) < 1e-4 * max(1.0, abs(ref[i].item())), (k, got, ref[i].item())
    # scene-flow columns with the disparity change derived from flow + occlusion
    kw2 = dict(gt_disp=d(disp), gt_flow=d(flow), gt_flow_occ=d(focc))
    row2 = est(img=d(left), r_img=d(right), img_metas=metas, return_loss=False, evaluate=True, **kw2)[0]
    assert float(row2["count"][0]) > 0 and float(row2["epe2d_scene_flow"][0]) > 0


def test_cli_folder_of_frames_writes_disparities(tmp_path):
    """codd_amd.inference on a folder of PNG frames == the estimator called on the same pre-processed
    tensors (reference inference.py --img-dir/--r-img-dir/--show)."""
    import numpy as np
    from PIL import Image
    from codd_amd import configs, inference, ops, synth
    from codd_amd.registry import build_estimator
    h, w, MF = 120, 250, 3
    left, right, _ = synth.stereo_sequence(h, w, MF, 24.0)
    for side, seq in (("l", left), ("r", right)):
        os.makedirs(tmp_path / side / "clip7")
        for f in range(MF):
            u8 = ((seq[0, f] - seq.min()) / (seq.max() - seq.min()) * 255).permute(1, 2, 0).byte().numpy()
            Image.fromarray(u8).save(tmp_path / side / "clip7" / ("%04d.png" % f))
    out_dir = tmp_path / "out"
    inference.main(["--img-dir", str(tmp_path / "l"), "--r-img-dir", str(tmp_path / "r"), "--iters", "2", "--show",
                    "--show-dir", str(out_dir), "--no-autotune"])
    got = np.load(out_dir / "clip7.disp.pred.npz")["disp"]
    assert got.shape == (MF, h, w) or got.shape == (1, MF, h, w)
    est = build_estimator(configs.codd(iters=2)).to(DEV).eval()
    synth.load_synthetic_weights(est, gain=1.4)
    vids = inference.list_videos(str(tmp_path / "l"), str(tmp_path / "r"), ".png")
    data = inference.make_sample(*vids[0], torch.device(DEV))
    assert data["img"][0].shape == (1, MF, 3, 128, 256)
    ref = est(return_loss=False, evaluate=False, **data)[0].cpu().numpy()
    assert np.array_equal(got.reshape(ref.shape), ref)


def test_ablation_plugins_match_oracle_and_golden():
    """KalmanFusion / GTFusion / GTMotion through the registry: bit-exact against the CPU restatement and
    the reference's own outputs (tests/golden ablation_* arrays)."""
    import numpy as np
    sys_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    import sys
    sys.path.insert(0, sys_path)
    import cases
    from codd_amd.registry import MODELS
    from oracle import ablation as oab
    G = np.load(os.path.join(sys_path, "reference_outputs.npz"))
    c = {k: v.to(DEV) for k, v in cases.ablation_case().items()}
    mem5 = [c["img_prev"], c["feat_prev"], torch.ones(1, 3, 32, 48, device=DEV), c["warp"], torch.zeros(1, 3, 32, 48, device=DEV)]
    kf = MODELS.build(dict(type="KalmanFusion"))
    o = dict(pred_disp=c["pred"].clone())
    kf.memory_query(o, dict(memory=mem5))
    assert torch.equal(o["pred_disp"].cpu(), torch.from_numpy(G["ablation_kalman"]))
    assert torch.equal(o["pred_disp"].cpu(), oab.kalman_fuse(c["pred"].cpu(), c["warp"].cpu()))
    o = dict(pred_disp=c["pred"].clone())
    MODELS.build(dict(type="GTFusion")).memory_query(o, dict(memory=mem5, gt_disp=[c["gt"]]))
    assert torch.equal(o["pred_disp"].cpu(), torch.from_numpy(G["ablation_gtfusion"]))
    st = dict(memory=[c["img_prev"], c["feat_prev"], c["disp_prev"]], gt_disp_change=[c["gt_disp_change"]],
              gt_flow=[c["gt_flow"]], gt_flow_occ=[c["gt_flow_occ"]])
    out = {}
    MODELS.build(dict(type="GTMotion"))(st, out, None)
    for t, k in zip(st["memory"], ("img", "feat", "conf", "disp", "flow")):
        assert torch.equal(t.cpu().reshape(G[f"ablation_gtmotion_{k}"].shape), torch.from_numpy(G[f"ablation_gtmotion_{k}"])), k
    assert out["Ts"].shape == (1, 32, 48, 7)
    nf = MODELS.build(dict(type="NullFusion"))
    s2 = {}
    nf.memory_update(dict(left_img=c["img_prev"], left_feat=c["left_feat"], pred_disp=c["pred"]), s2)
    assert len(s2["memory"]) == 3 and s2["memory"][2].shape == (1, 32, 48)


def test_metric_kernels_match_reference_calc_metric():
    """HIP metric kernels fed with the reference's own predictions reproduce the reference's metric dict
    (tests/golden metric_* arrays: model/codd.py:435-521 run in the build container)."""
    import numpy as np
    import sys
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    sys.path.insert(0, gdir)
    import cases
    from codd_amd import metrics
    G = np.load(os.path.join(gdir, "reference_outputs.npz"))
    img, r_img, gt, flow, meta = cases.metric_case()
    h, w = meta[0]["img_shape"][:2]
    H, W = img.shape[-2:]
    pred = torch.zeros(1, gt.shape[1], 1, H, W)
    pred[:, :, 0, :h, :w] = torch.from_numpy(G["metric_pred_disp"])
    sm = metrics.SequenceMetrics(meta[0], torch.device(DEV))
    pd, gd, fd = pred.to(DEV), gt.to(DEV), flow.to(DEV)
    for f in range(pred.shape[1]):
        sm.update_disparity_device(pd[:, f].contiguous(), gd[:, f].contiguous(), (h, w))
        if f > 0:
            sm.update_temporal_device(pd[:, f].contiguous(), gd[:, f].contiguous(), pd[:, f - 1].contiguous(),
                                      gd[:, f - 1].contiguous(), fd[:, f - 1].contiguous(), (h, w))
    row = sm.row().cpu()
    ref = G["metric_values"]
    for i, k in enumerate(metrics.COLUMNS[:7]):
        assert abs(row[i].item() - float(ref[i])) < 2e-5 * max(1.0, abs(float(ref[i]))), (k, row[i].item(), ref[i])


def test_metric_kernels_kitti_style_ground_truth():
    """The HIP metric kernels with KITTI-style ground truth (frame without disparity -> dummy mask source, gt_disp2,
    gt_disp_occ) against the reference's own metric dict (golden metric_kitti_values)."""
    import numpy as np
    import sys
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    sys.path.insert(0, gdir)
    import cases
    from codd_amd import metrics as M
    G = np.load(os.path.join(gdir, "reference_outputs.npz"))
    img, r_img, gt, flow, gt2, occ, meta = cases.kitti_metric_case()
    h, w = meta[0]["img_shape"][:2]
    H, W = img.shape[-2:]
    pred = torch.zeros(1, gt.shape[1], 1, H, W)
    pred[:, :, 0, :h, :w] = torch.from_numpy(G["metric_pred_disp"])
    sm = M.SequenceMetrics(meta[0], torch.device(DEV))
    pd, gd, fd, g2, seg = pred.to(DEV), gt.to(DEV), flow.to(DEV), gt2.to(DEV), (occ <= 0).to(DEV)
    F_ = lambda t, f: t[:, f].contiguous()
    for f in range(pred.shape[1]):
        gi = M.apply_seg(F_(gd, f), F_(seg, f))
        sm.update_disparity_device(F_(pd, f), gi, (h, w))
        if f > 0:
            sm.update_temporal_device(F_(pd, f), gi, F_(pd, f - 1), M.apply_seg(F_(gd, f - 1), F_(seg, f - 1)),
                                      F_(fd, f - 1), (h, w), gt_mask=M.temporal_mask_source(F_(gd, f), F_(seg, f)),
                                      gt2_prev=F_(g2, f - 1))
    row = sm.row().cpu()
    ref = G["metric_kitti_values"]
    for i, k in enumerate(M.COLUMNS[:7]):
        assert abs(row[i].item() - float(ref[i])) < 2e-5 * max(1.0, abs(float(ref[i]))), (k, row[i].item(), ref[i])


def test_fused_geometry_lookup_equals_separate_kernels():
    from codd_amd import ops
    h, w = 24, 40
    T = ops.se3_identity(1, h, w, DEV)
    T[..., :3] = rnd(1, h, w, 3, seed=3).to(DEV) * 0.05
    q = rnd(1, h, w, 4, seed=4).to(DEV) * 0.05
    q[..., 3] = 1.0
    T[..., 3:] = q / q.norm(dim=-1, keepdim=True)
    d1 = (rnd(1, h, w, seed=5).abs() * 5 + 2).to(DEV)
    d2 = (rnd(1, h, w, seed=6).abs() * 5 + 2).to(DEV)
    pyr = ops.allpairs_corr(rnd(1, 128, h, w, seed=7).to(DEV), rnd(1, 128, h, w, seed=8).to(DEV))
    K8 = [30.0, 32.0, 20.0, 12.0]
    xyz, minfo = ops.raft_geometry(T, d1, d2, K8)
    corr = ops.corr_lookup(pyr, xyz, h, w)
    xyz2, minfo2, corr2 = ops.raft_geometry_lookup(T, d1, d2, K8, pyr)
    assert torch.equal(xyz, xyz2) and torch.equal(minfo, minfo2)
    assert (corr - corr2).abs().max().item() < 1e-5 * max(1.0, corr.abs().max().item())


def test_gru_gates_writing_split_records_equal_gate_plus_relayout():
    """codd_gru_gate_zr_xs / codd_gru_gate_q_xs (gate fused with the re-layout of its result into the next
    convolution's split-bf16 input) == the plain gate kernels followed by codd_split_bf16, bit for bit."""
    from codd_amd import ops
    B, h, w = 1, 23, 37
    t1, t2 = rnd(B, 256, h, w, seed=1).to(DEV), rnd(B, 256, h, w, seed=2).to(DEV)
    inp, cor, mot = (rnd(B, 384, h, w, seed=s).to(DEV) for s in (3, 4, 5))
    net = torch.tanh(rnd(B, 128, h, w, seed=6)).to(DEV)
    zr, rh = ops.gru_gate_zr(t1, t2, inp, cor, mot, net)
    rs = ops.split_buffer(("test", "rh"), B, 128, h, w, 4, DEV)
    z = ops.gru_gate_zr_xs(t1, t2, inp, cor, mot, net, rs)
    assert torch.equal(z, zr[:, :128])
    ref = ops.split_input(rh, border=4)
    assert (ref.c8, ref.hp, ref.wp) == (rs.c8, rs.hp, rs.wp) and torch.equal(ref.buf, rs.buf)
    q1, q2 = rnd(B, 128, h, w, seed=7).to(DEV), rnd(B, 128, h, w, seed=8).to(DEV)
    h_ref = ops.gru_gate_q(q1, q2, inp, cor, mot, zr, net)
    hb = ops.split_buffer(("test", "net"), B, 128, h, w, 4, DEV)
    h_new = ops.gru_gate_q_xs(q1, q2, inp, cor, mot, z, net, hb)
    assert torch.equal(h_new, h_ref)
    assert torch.equal(ops.split_input(h_ref, border=4).buf, hb.buf)


@pytest.mark.parametrize("mode,wtol,ttol", [("split", 1e-4, 2e-3), ("split16", 1e-4, 2e-3), ("fp16", 4e-3, 6e-2)])
def test_gn_step_with_fused_heads_equals_heads_then_step(mode, wtol, ttol):
    """codd_se3_gn_step_heads (1x1 heads inside the record packing, hidden channels read in split-bf16 form -- or, mode
    "fp16", as one plane of IEEE fp16 records with fp16 head weights on v_mfma_f32_16x16x32_f16) against fp32 1x1
    convolutions (torch) followed by codd_se3_gn_step."""
    from codd_amd import ops
    prev = ops.set_conv_precision(mode)
    try:
        _gn_step_with_fused_heads(ops, mode, wtol, ttol)
    finally:
        ops.set_conv_precision(prev)


def _gn_step_with_fused_heads(ops, mode, wtol, ttol):
    B, h, w = 1, 20, 44
    T = _se3_field(B, h, w, 0.03).to(DEV)
    g = torch.Generator().manual_seed(11)
    d1 = (torch.rand(B, h, w, generator=g) * 30 + 3).to(DEV)
    K8 = [40.0, 42.0, w / 2.0, h / 2.0]
    xyz = (torch.rand(B, h, w, 3, generator=g) * 20).to(DEV)
    hidden = torch.relu(rnd(B, 768, h, w, seed=12)).to(DEV)
    Wm = (rnd(38, 256, seed=13) / 16).to(DEV)
    bm = (rnd(38, seed=14) * 0.1).to(DEV)
    hs = ops.split_input(hidden, border=0)
    assert hs is not None, "needs the split / bf16 conv precision (the default)"
    grp = lambda i: hidden[:, 256 * i:256 * (i + 1)]
    ae = F.conv2d(grp(0), Wm[:32, :, None, None], bm[:32])
    delta = F.conv2d(grp(1), Wm[32:35, :, None, None], bm[32:35])
    weight = torch.sigmoid(F.conv2d(grp(2), Wm[35:38, :, None, None], bm[35:38]))
    T_ref = T.clone()
    ops.se3_gn_step(T_ref, ae.contiguous(), xyz, delta.contiguous(), weight.contiguous(), d1, K8, radius=6)
    T_new = T.clone()
    from codd_amd.motion import pack_head_matrix
    assert hs.terms == ops._TERMS[mode]
    w_out = ops.se3_gn_step_heads(T_new, hs, pack_head_matrix(Wm, f16=mode in ("fp16", "split16")), bm, xyz, d1, K8, radius=6)
    step = (T_ref - T).abs().max().item()
    err = (T_new - T_ref).abs().max().item()
    print(mode, "gn step", step, "fused-heads deviation", err, "weight dev", (w_out - weight).abs().max().item())
    assert (w_out - weight).abs().max().item() < wtol
    assert err < ttol * step


@pytest.mark.parametrize("mode", ["split", "split16", "fp16"])
def test_geometry_lookup_writing_split_records_equals_lookup_plus_relayout(mode):
    """(mode "fp16": the same writers emit one plane of IEEE fp16 records, CODD_TERMS_F16)"""
    from codd_amd import ops
    prev = ops.set_conv_precision(mode)
    try:
        _geometry_lookup_records(ops)
    finally:
        ops.set_conv_precision(prev)


def _geometry_lookup_records(ops):
    h, w = 24, 40
    T = ops.se3_identity(1, h, w, DEV)
    T[..., :3] = rnd(1, h, w, 3, seed=3).to(DEV) * 0.05
    q = rnd(1, h, w, 4, seed=4).to(DEV) * 0.05
    q[..., 3] = 1.0
    T[..., 3:] = q / q.norm(dim=-1, keepdim=True)
    d1 = (rnd(1, h, w, seed=5).abs() * 5 + 2).to(DEV)
    d2 = (rnd(1, h, w, seed=6).abs() * 5 + 2).to(DEV)
    pyr = ops.allpairs_corr(rnd(1, 128, h, w, seed=7).to(DEV), rnd(1, 128, h, w, seed=8).to(DEV))
    K8 = [30.0, 32.0, 20.0, 12.0]
    xyz, minfo, corr = ops.raft_geometry_lookup(T, d1, d2, K8, pyr)
    cxs = ops.split_buffer(("test", "corr_in"), 1, 196, h, w, 1, DEV)
    mxs = ops.split_buffer(("test", "minfo_in"), 1, 9, h, w, 3, DEV)
    xyz2, m2, c2 = ops.raft_geometry_lookup(T, d1, d2, K8, pyr, minfo_xs=mxs, corr_xs=cxs)
    assert m2 is None and c2 is None and torch.equal(xyz, xyz2)
    assert torch.equal(ops.split_input(corr, border=1).buf, cxs.buf)
    assert torch.equal(ops.split_input(minfo, border=3).buf, mxs.buf)


def test_full_codd_parity_with_autotuned_launch_configurations():
    """The configurations the tuner picks (quad-layout kernel, 2/8/9-wave workgroups, ...) in the whole pipeline:
    HIP vs oracle on a 3-frame sequence, same bound as the un-tuned parity tests."""
    from codd_amd import configs, ops, synth
    from codd_amd.registry import build_estimator
    from oracle import codd as oc
    H, W, MF, iters = 128, 256, 3, 2
    est = build_estimator(configs.codd(iters=iters)).eval()
    synth.load_synthetic_weights(est, 1.4)
    sd = {k: v.clone() for k, v in est.state_dict().items()}
    est = est.to(DEV)
    img, r_img, _ = synth.stereo_sequence(H, W, MF, 32.0)
    intr = (160.0, 160.0, 128.0, 64.0)
    metas = synth.default_metas(H, W, intrinsics=intr)[0]
    so, sg = {}, {}
    ops.enable_autotune(True, shipped=False)
    try:
        with torch.no_grad():
            for f in range(MF):
                oo = oc.frame(sd, img[:, f], r_img[:, f], so, intr, iters=iters)
                og = est.consistent_online_depth_estimation(img[:, f].to(DEV).contiguous(), r_img[:, f].to(DEV).contiguous(),
                                                            metas, sg)
                d = (og["pred_disp"].cpu() - oo["pred_disp"]).abs()
                print(f"tuned frame {f}: mean {d.mean().item():.3e}  >1e-2 px: {(d > 1e-2).float().mean().item():.2e}")
                assert d.median().item() < 1e-4 and (d > 1e-2).float().mean().item() < 2e-3, (f, d.mean().item())
                assert d[d <= 1e-2].mean().item() < 1e-3
    finally:
        ops.enable_autotune(False)
    assert len(ops.TUNE_DB) > 50


def test_graph_inference_follows_weight_and_policy_changes(tmp_path):
    """estimator.inference(use_graph=True) caches captured frame graphs on the model.  A graph bakes in the packed
    weights, so after apis.load_checkpoint (new weights), a precision change or an in-place weight edit the next
    inference must NOT replay the stale graph: every result has to equal the eager path run under the same policy.
    Also: the cache is bounded, keyed by batch size, and does not break copy / pickling of the model."""
    import copy
    from codd_amd import apis, configs, ops, synth
    from codd_amd.registry import build_estimator
    H, W, MF = 128, 192, 3
    est = build_estimator(configs.codd(iters=2)).to(DEV).eval()
    synth.load_synthetic_weights(est, gain=1.4)
    left, right, _ = synth.stereo_sequence(H, W, MF, 24.0)
    metas = synth.default_metas(H, W)
    d = lambda t: [t.to(DEV)]

    def run(graph):
        est.use_graph = graph
        return est(img=d(left), r_img=d(right), img_metas=metas, return_loss=False, evaluate=False)[0].clone()

    g0, e0 = run(True), run(False)
    assert (g0 - e0).abs().max().item() < 1e-4
    # new weights through the checkpoint loader
    other = build_estimator(configs.codd(iters=2)).eval()
    synth.load_synthetic_weights(other, gain=1.1)
    torch.save(dict(state_dict=other.state_dict()), str(tmp_path / "w2.pth"))
    apis.load_checkpoint(est, str(tmp_path / "w2.pth"), strict=True)
    g1, e1 = run(True), run(False)
    assert (g1 - e1).abs().max().item() < 1e-4
    assert (g1 - g0).abs().mean().item() > 1e-3, "the second checkpoint must change the result"
    # an in-place edit without the loader (the weights token of the runner key notices it)
    with torch.no_grad():
        est.stereo.tile_update.tile_update6.lastconv.weight.mul_(0.5)
    g2, e2 = run(True), run(False)
    assert (g2 - e2).abs().max().item() < 1e-4 and (g2 - g1).abs().mean().item() > 1e-4
    # precision policy
    prev = ops.set_conv_precision("fp32")
    try:
        g3, e3 = run(True), run(False)
    finally:
        ops.set_conv_precision(prev)
    assert (g3 - e3).abs().max().item() < 1e-4
    assert len(est._runners) <= est.RUNNER_CACHE
    copy.deepcopy(est)  # captured graphs are not part of the model's state
    assert "_runners" not in est.__getstate__()


def test_scene_flow_evaluation_through_graph_replay_equals_eager():
    """inference(evaluate=True) with gt_disp_change: the scene-flow columns read the SE3 field of every frame; under
    use_graph it comes from the captured graph's static output (FrameRunner.last["Ts"]) and the row must equal the
    eager one."""
    from codd_amd import configs, metrics as M, synth
    from codd_amd.registry import build_estimator
    H, W, MF = 128, 192, 3
    est = build_estimator(configs.codd(iters=2)).to(DEV).eval()
    synth.load_synthetic_weights(est, gain=1.4)
    left, right, disp = synth.stereo_sequence(H, W, MF, 24.0)
    metas = synth.default_metas(H, W)
    metas[0][0].update(disp_range=(1, 210))
    flow = rnd(1, MF, 2, H, W, seed=5) * 2
    dc = rnd(1, MF, 1, H, W, seed=6) * 0.5
    d = lambda t: [t.to(DEV)]
    kw = dict(gt_disp=d(disp), gt_flow=d(flow), gt_disp_change=d(dc))
    rows = []
    for graph in (False, True):
        est.use_graph = graph
        rows.append(est(img=d(left), r_img=d(right), img_metas=metas, return_loss=False, evaluate=True, **kw)[0])
    assert est._runners, "the graph path must have been taken"
    assert float(rows[1]["count"][0]) > 0
    for k in M.COLUMNS:
        a, b = float(rows[0][k][0]), float(rows[1][k][0])
        assert abs(a - b) <= 1e-4 * max(1.0, abs(a)), (k, a, b)


@pytest.mark.parametrize("patch", [3, 5])
def test_fused_forget_branch_equals_cues_plus_head_convolutions(patch):
    """codd_fusion_forget (cues + merged linear forget head + sigmoid in one launch; the cue tensor is never written)
    against torch on the materialised cue tensor of codd_fusion_cues_fr -- layer by layer, as the reference evaluates
    forget_head (fusion.py:123-132) -- incl. image borders (the 3x3's zero padding acts on the BIASED 16-channel map),
    warped-disparity holes and a map that is not a multiple of the 16x16 tile."""
    from codd_amd import configs, ops, synth
    from codd_amd.registry import MODELS
    H, W = 50, 77
    cfg = dict(configs.codd(iters=2)["fusion"])
    cfg["corr_cfg"] = dict(cfg.get("corr_cfg", {}), patch_size=patch)
    fus = MODELS.build(cfg).to(DEV).eval()
    g = torch.Generator().manual_seed(patch)
    for prm in fus.forget_head.parameters():
        prm.data = (torch.randn(prm.shape, generator=g) * 0.3).to(DEV)
    pc = (rnd(1, 1, H, W, seed=1).abs() * 20 + 1).to(DEV)
    pw = (rnd(1, 1, H, W, seed=2).abs() * 20 + 1)
    pw[:, :, 10:20, 30:44] = 0.0  # holes of the warped disparity
    pw = pw.to(DEV)
    flow, conf = rnd(1, 3, H, W, seed=3).to(DEV), rnd(1, 3, H, W, seed=4).abs().to(DEV)
    cues = ops.fusion_cues_fr(pc, pw, flow, conf, patch=patch).cpu()
    fh = fus.forget_head.cpu()
    ref = torch.sigmoid(fh[2](fh[1](fh[0](cues))))
    fus.forget_head.to(DEV)
    got = ops.fusion_forget(pc, pw, flow, conf, fus.forget_matrix(), patch=patch).cpu()
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() < 2e-5, (got - ref).abs().max().item()


def _records_of(st):
    """SplitTensor -> fp32 NCHW of its image interior (hi + lo planes)."""
    planes = 2 if st.terms == 3 else 1
    rec = st.buf.view(torch.bfloat16).view(st.B, planes, st.c8, st.hp, st.wp, 8).float().sum(1)
    img = rec[:, :, st.bt:st.bt + st.H, st.bl:st.bl + st.W]            # [B, c8, H, W, 8]
    return img.permute(0, 1, 4, 2, 3).reshape(st.B, st.c8 * 8, st.H, st.W)[:, :st.C]


@pytest.mark.parametrize("hw", [(23, 37), (72, 120)])
def test_gate_epilogue_convolutions_against_torch(hw):
    """codd_conv_params.gate / dil2 (ops.conv_gate): the dual-tap-set z|r convolution into a channel-quad tensor, the
    merged gate-input 1x1 convolution ending in the z / r*h / q-input epilogue, and the dual-tap-set q convolution
    ending in the state update -- against torch fp32 convolutions + the ConvGRU formulas (blocks/gru.py:17-34)."""
    from codd_amd import ops
    from codd_amd.motion import packed_dual
    B, (h, w) = 1, hw
    net = torch.tanh(rnd(B, 128, h, w, seed=1))
    ctx = torch.relu(rnd(B, 384, h, w, seed=2))
    enc = torch.relu(rnd(B, 384, h, w, seed=3))
    mk = lambda cout, cin, k, s: (rnd(cout, cin, k, k, seed=s) / (cin * k * k) ** 0.5, rnd(cout, seed=s + 50) * 0.1)
    (wz1, bz1), (wz2, bz2), (wr1, br1), (wr2, br2) = mk(128, 128, 3, 11), mk(128, 128, 3, 12), mk(128, 128, 3, 13), mk(128, 128, 3, 14)
    (wq1, bq1), (wq2, bq2), (wm, bm) = mk(128, 128, 3, 15), mk(128, 128, 3, 16), mk(384, 384, 1, 17)
    conv = lambda x, wt, b, d: F.conv2d(x, wt, b, padding=d, dilation=d)
    t12_ref = torch.cat([conv(net, wz1, bz1, 1) + conv(net, wz2, bz2, 4), conv(net, wr1, br1, 1) + conv(net, wr2, br2, 4)], 1)
    s = F.conv2d(enc, wm, bm) + ctx
    z_ref = torch.sigmoid(s[:, :128] + t12_ref[:, :128])
    rh_ref = torch.sigmoid(s[:, 128:256] + t12_ref[:, 128:]) * net
    q_ref = torch.tanh(conv(rh_ref, wq1, bq1, 1) + conv(rh_ref, wq2, bq2, 4) + s[:, 256:])
    h_ref = (1 - z_ref) * net + z_ref * q_ref

    class M:  # stand-ins for nn.Conv2d as packed_dual reads them
        def __init__(self, wt, b):
            self.weight, self.bias = wt.to(DEV), b.to(DEV)
    key = ("gate_test", h, w)
    ns = ops.split_input(net.to(DEV), border=4)
    es = ops.split_input(enc.to(DEV), border=0)
    assert ns is not None and es is not None, "needs the split / bf16 conv precision (the default)"
    t12 = ops.c4_buffer((key, "t12"), B, 256, h, w, DEV)
    ops.conv_gate(packed_dual(((M(wz1, bz1), M(wz2, bz2)), (M(wr1, br1), M(wr2, br2)))), ns, 1, pad=4, dil=4, dil2=1, out=t12)
    assert rel(t12.nchw().cpu(), t12_ref) < 2e-5
    ctx4 = ops.to_c4(ctx.to(DEV), ops.c4_buffer((key, "ctx"), B, 384, h, w, DEV))
    h4 = ops.to_c4(net.to(DEV), ops.c4_buffer((key, "h4"), B, 128, h, w, DEV))
    assert torch.equal(h4.nchw().cpu(), net)
    zq = ops.c4_buffer((key, "zq"), B, 256, h, w, DEV)
    rs = ops.split_buffer((key, "rh"), B, 128, h, w, 4, DEV)
    hb = ops.split_buffer((key, "net"), B, 128, h, w, 4, DEV)
    pm = ops.PackedConv(wm.to(DEV), bm.to(DEV))
    ops.conv_gate(pm, es, 2, out=zq, res1=ctx4, res2=t12, post=h4, xs_out=rs)
    got = zq.nchw().cpu()
    assert rel(got[:, :128], z_ref) < 2e-5 and rel(got[:, 128:], s[:, 256:]) < 2e-5
    assert rel(_records_of(rs).cpu(), rh_ref) < 2e-5
    ops.conv_gate(packed_dual(((M(wq1, bq1), M(wq2, bq2)),)), rs, 3, pad=4, dil=4, dil2=1, out=h4, res1=zq, post=h4, xs_out=hb)
    assert rel(h4.nchw().cpu(), h_ref) < 5e-5
    assert rel(_records_of(hb).cpu(), h_ref) < 5e-5
    # the borders of the persistent record tensors stay zero
    full = hb.buf.view(torch.bfloat16).view(B, -1, hb.c8, hb.hp, hb.wp, 8).float()
    assert full[:, :, :, :hb.bt].abs().max().item() == 0 and full[:, :, :, :, :hb.bl].abs().max().item() == 0


def test_update_block_with_fused_gates_equals_gate_kernels():
    """BasicUpdateBlock.run with the gates as convolution epilogues (CODD_FUSE_GATES) against the same block with the
    separate gate kernels and conv*1 / conv*2 launches: three chained updates, hidden state and head outputs."""
    from codd_amd import motion, ops
    B, h, w = 1, 24, 40
    torch.manual_seed(3)
    outs = {}
    for fused in (False, True):
        prev = motion.FUSE_GATES
        motion.FUSE_GATES = fused
        try:
            ub = motion.BasicUpdateBlock().to(DEV).eval()
            g = torch.Generator().manual_seed(5)
            with torch.no_grad():
                for p_ in ub.parameters():
                    p_.copy_((torch.randn(p_.shape, generator=g) * (0.5 / max(1, p_[0].numel()) ** 0.5)).to(DEV))
            net = torch.tanh(rnd(B, 128, h, w, seed=1)).to(DEV)
            inp = torch.relu(rnd(B, 384, h, w, seed=2)).to(DEV)
            cxs, mxs = ub.input_buffers(net)
            assert cxs is not None
            zr, res = None, []
            for it in range(3):
                corr, minfo = rnd(B, 196, h, w, seed=10 + it).to(DEV), rnd(B, 9, h, w, seed=20 + it).to(DEV)
                ops.split_input(corr, border=1, out=cxs)
                ops.split_input(minfo, border=3, out=mxs)
                net, mask, ae, delta, weight, zr, hid = ub.run(net, inp, None, None, need_mask=it == 2, zr=zr,
                                                               prefetch_next=it < 2, fuse_heads=True)
                torch.cuda.synchronize()
                res.append((_records_of(ub._xs[1]).cpu(), _records_of(hid).cpu(), None if mask is None else mask.cpu()))
            outs[fused] = res
        finally:
            motion.FUSE_GATES = prev
    for it, (a, b) in enumerate(zip(outs[False], outs[True])):
        assert rel(b[0], a[0]) < 1e-4, it       # hidden state
        assert rel(b[1], a[1]) < 1e-4, it       # head hidden channels
        if a[2] is not None:
            assert rel(b[2], a[2]) < 1e-4


def _gn_two_steps(ops):
    g = torch.Generator().manual_seed(5)
    B, h, w = 2, 37, 61
    T = torch.zeros(B, h, w, 7); T[..., 6] = 1; T[..., :3] = torch.randn(B, h, w, 3, generator=g) * 0.02
    d1 = torch.rand(B, h, w, generator=g) * 30 + 3
    ae = torch.randn(B, 32, h, w, generator=g) * 3
    xyz = torch.rand(B, h, w, 3, generator=g) * 40
    delta = torch.randn(B, 3, h, w, generator=g) * 0.2
    wgt = torch.sigmoid(torch.randn(B, 3, h, w, generator=g))
    Tg = T.to(DEV)
    for _ in range(2):
        ops.se3_gn_step(Tg, ae.to(DEV), xyz.to(DEV), delta.to(DEV), wgt.to(DEV), d1.to(DEV), [40.0, 42.0, w / 2.0, h / 2.0], radius=32)
    return Tg.cpu()


def test_se3_gn_pair_builder_with_embedding_in_lds_is_bit_identical():
    """se3_gn_build_kernel<true> (the shipped builder: the pixel's own embedding read from LDS instead of 32 registers, four
    waves per SIMD) issues the pair builder's instructions on the same values in the same order as se3_gn_build_kernel<false>
    (CODD_OPT_GN_BUILDER = 3, kept as its reference): torch.equal on the updated field."""
    from codd_amd import _abi, ops
    outs = []
    try:
        for builder in (3, 5):
            _abi.set_option("gn_builder", builder)
            outs.append(_gn_two_steps(ops))
    finally:
        _abi.set_option("gn_builder", 5)
    assert torch.isfinite(outs[0]).all() and (outs[0][..., :3].abs().max().item() > 1e-3)
    assert torch.equal(outs[0], outs[1]), (outs[0] - outs[1]).abs().max().item()


def test_library_options_replace_environment_switches():
    """codd_set_option / codd_get_option (ABI v12): defaults = the shipped configuration, bad keys / values are rejected, the
    previous value comes back, and another Gauss-Newton grouping (CODD_OPT_GN_Q4: another fp32 summation order of the same
    normal equations, with another scratch size) gives the same step to rounding level."""
    from codd_amd import _abi, ops
    lib = _abi.load()
    assert lib.codd_get_option(0) == 192 and lib.codd_get_option(1) == 5
    assert lib.codd_set_option(99, 1) < 0 and lib.codd_set_option(0, 3) < 0 and lib.codd_set_option(1, 4) < 0
    assert lib.codd_get_option(99) < 0
    s192 = lib.codd_se3_gn_scratch(1, 72, 120, 32)
    ref = _gn_two_steps(ops)
    try:
        assert _abi.set_option("gn_q4", 256) == 192
        assert lib.codd_se3_gn_scratch(1, 72, 120, 32) != s192
        got = _gn_two_steps(ops)
    finally:
        assert _abi.set_option("gn_q4", 192) == 256
    d = (got - ref).abs().max().item()
    assert 0 <= d < 2e-5 * ref.abs().max().item(), d


def test_resize_bilinear_add_equals_two_launches():
    """codd_resize_bilinear_add (the '+ x_i' term of an HRModule fuse layer folded into the neighbouring up-sampling
    term) against the two launches it replaces (add_relu, then resize_bilinear with accumulate): the same bits."""
    from codd_amd import ops
    g = torch.Generator().manual_seed(5)
    for (C, H, W, s) in [(18, 72, 120, 2), (36, 36, 60, 4), (7, 10, 14, 2)]:
        acc0 = (torch.randn(1, C, H, W, generator=g) * 30).to(DEV)
        xi = (torch.randn(1, C, H, W, generator=g) * 30).to(DEV)
        t = (torch.randn(1, C, H // s, W // s, generator=g) * 30).to(DEV)
        for accumulate in (True, False):
            for relu in (True, False):
                a = acc0.clone()
                ops.add_relu(xi, a if accumulate else None, relu=False, out=a)
                ops.resize_bilinear(t, (H, W), False, out=a, accumulate=True, relu=relu)
                b = acc0.clone()
                ops.resize_bilinear(t, (H, W), False, out=b, accumulate=accumulate, relu=relu, extra=xi)
                assert torch.equal(a, b), (C, H, W, s, accumulate, relu, (a - b).abs().max().item())


def test_deferred_convs_equal_single_launches():
    """ops.deferred_convs(): independent convolutions of the multi-job class leave as codd_conv2d_multi launches with the
    parameters of their single launches -- bit-identical outputs, residual / output-slice operands included; convolutions
    of other classes inside the block launch at once."""
    from codd_amd import ops
    from codd_amd.ops import Slice
    prev = ops.set_conv_precision("fp32")
    try:
        g = torch.Generator().manual_seed(9)
        jobs = []
        for (cin, cout, k, st, H, W) in [(18, 18, 3, 2, 72, 120), (36, 18, 1, 1, 36, 60), (72, 36, 1, 1, 36, 60),
                                         (64, 16, 1, 1, 36, 60), (18, 36, 3, 2, 72, 120), (24, 24, 3, 1, 9, 15)]:
            x = torch.randn(1, cin, H, W, generator=g).to(DEV)
            w = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(DEV)
            pc = ops.PackedConv(w, (torch.randn(cout, generator=g) * 0.1).to(DEV))
            Ho, Wo = (H + 2 * (k // 2) - k) // st + 1, (W + 2 * (k // 2) - k) // st + 1
            res = torch.randn(1, cout, Ho, Wo, generator=g).to(DEV)
            pc.tuned[(Ho, Wo, 1, st, st, 1, 1, k // 2, False, 0)] = (1, 4, 16 if cin <= 16 or k == 3 else 32, 1, 1)
            jobs.append((x, pc, st, k // 2, res, cout, Ho, Wo))

        def run():
            outs = []
            for x, pc, st, pad, res, cout, Ho, Wo in jobs:
                buf = torch.full((1, cout + 2, Ho, Wo), 3.0, device=DEV)
                ops.conv2d(x, pc, stride=st, pad=pad, act="relu", res1=res, out=Slice(buf, 1, cout))
                outs.append(buf)
            return outs

        single = run()
        with ops.deferred_convs():
            batched = run()
        torch.cuda.synchronize()
        for a, b in zip(single, batched):
            assert torch.equal(a, b)
    finally:
        ops.set_conv_precision(prev)


def test_timestamp_marks_are_ordered():
    """codd_timestamp (diagnostics, ABI v9): two marks around a launch on one stream are ordered, 100 MHz ticks."""
    from codd_amd import ops
    marks = torch.zeros(4, dtype=torch.int64, device=DEV)
    ops.timestamp(marks, 0)
    x = torch.randn(1 << 22, device=DEV)
    for _ in range(20):
        x = x * 1.0001
    ops.timestamp(marks, 1)
    torch.cuda.synchronize()
    t0, t1 = marks[0].item(), marks[1].item()
    assert t0 > 0 and 0 < t1 - t0 < 100e6 * 5  # (positive, and less than five seconds of ticks)
