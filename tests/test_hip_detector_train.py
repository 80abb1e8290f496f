"""GPU tests of the LiDAR backbone pretraining (stage 1 of the reference's recipe): the fused detector loss (csrc/loss.hip) against
torch autograd in float64, the standalone PointPillar detector in training mode, the stage-1 -> stage-2 hand-over through the
trainer's CLI, late-fusion replay of a stage-1 checkpoint, and one stage-1 step at the shipped size."""
import copy
import json
import math
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, rel_max_err

sys.path.insert(0, GOLDEN)

pytestmark = pytest.mark.gpu


def _loss_case(scale, seed=5):
    """Stage-1 label map (128 x 128 x 2 anchors, B = 8) from generate_label, a few boxes per sample, sample 3 without positives,
    a few NaN targets in channels 0-5; logits uniform in +-scale."""
    import hmvit_amd  # noqa: F401
    from hmvit_amd import replay as R
    from hmvit_amd.postprocess import VoxelPostprocessor
    cfg = R.lidar_model_config(512, 512)
    post = VoxelPostprocessor(R.postprocess_params(cfg), train=True)
    anchors = post.generate_anchor_box()
    rs = np.random.RandomState(seed)
    labels = []
    for b in range(8):
        n = 0 if b == 3 else rs.randint(2, 6)
        center = np.zeros((16, 7), np.float32)
        mask = np.zeros(16, np.float32)
        for i in range(n):
            center[i] = [rs.uniform(-90, 90), rs.uniform(-90, 90), -1.0, 1.56, 1.6, 3.9, rs.uniform(-math.pi, math.pi)]
            mask[i] = 1
        labels.append(post.generate_label(gt_box_center=center, anchors=anchors, mask=mask))
    tgt = VoxelPostprocessor.collate_batch(labels)
    tgt = {k: v.float() for k, v in tgt.items()}
    tgt["targets"][1, 5, 7, 2] = float("nan")
    tgt["targets"][6, 60, 61, 7 + 4] = float("nan")
    B, H, W, A = tgt["pos_equal_one"].shape
    g = torch.Generator().manual_seed(seed)
    psm = (torch.rand(B, A, H, W, generator=g) * 2 - 1) * scale
    rm = torch.randn(B, 7 * A, H, W, generator=g) * 0.5
    assert (H, W, A) == (128, 128, 2)
    pos = tgt["pos_equal_one"].sum((1, 2, 3))
    assert pos[3] == 0 and bool((pos[torch.arange(8) != 3] > 0).all())
    return psm, rm, tgt


def _torch_reference(psm, rm, tgt):
    from hmvit_amd.train import PointPillarLoss
    p = psm.double().requires_grad_(True)
    r = rm.double().requires_grad_(True)
    crit = PointPillarLoss({"cls_weight": 1.0, "reg": 2.0})
    total = crit({"psm": p, "rm": r}, {k: v.double() for k, v in tgt.items()})
    total.backward()
    return {k: float(v.detach()) for k, v in crit.loss_dict.items()}, p.grad, r.grad


def _fused(psm, rm, tgt):
    from hmvit_amd import FusedPointPillarLoss
    p = psm.cuda().requires_grad_(True)
    r = rm.cuda().requires_grad_(True)
    crit = FusedPointPillarLoss({"cls_weight": 1.0, "reg": 2.0})
    total = crit({"psm": p, "rm": r}, {k: v.cuda() for k, v in tgt.items()})
    total.backward()
    return {k: v.detach().clone() for k, v in crit.loss_dict.items()}, p.grad.detach().clone(), r.grad.detach().clone()


@pytest.mark.parametrize("scale", [80.0, 2.0])
def test_fused_loss_matches_torch_autograd_in_float64(scale):
    psm, rm, tgt = _loss_case(scale)
    ref, dp_ref, dr_ref = _torch_reference(psm, rm, tgt)
    got, dp, dr = _fused(psm, rm, tgt)
    for k in ("total_loss", "conf_loss", "reg_loss"):
        v = float(got[k])
        assert math.isfinite(v) and abs(v - ref[k]) <= 1e-5 * abs(ref[k]), (k, v, ref[k])
    assert bool(torch.isfinite(dp).all()) and bool(torch.isfinite(dr).all())
    assert rel_max_err(dp.cpu(), dp_ref) < 1e-5
    assert rel_max_err(dr.cpu(), dr_ref) < 1e-5
    assert float(dp[3].abs().max()) > 0                               # the sample without positives still has its negatives' gradient
    # fixed-order reductions: a second call gives the same bits
    got2, dp2, dr2 = _fused(psm, rm, tgt)
    assert all(torch.equal(got[k], got2[k]) for k in got)
    assert torch.equal(dp, dp2) and torch.equal(dr, dr2)


def test_fused_loss_matches_reference_golden_and_scales_by_grad_output():
    """The reference's own loss values (golden g14, frozen from the imported reference), and backward(c) = c * gradient."""
    from make_goldens_inputs import loss_inputs
    from hmvit_amd import FusedPointPillarLoss
    g = load_golden("g14_loss.npz")
    psm, rm, tgt = loss_inputs()
    p = psm.cuda().requires_grad_(True)
    r = rm.cuda().requires_grad_(True)
    crit = FusedPointPillarLoss({"cls_weight": 1.0, "reg": 2.0})
    total = crit({"psm": p, "rm": r}, {k: v.cuda() for k, v in tgt.items()})
    (3.0 * total).backward()
    assert abs(float(total.detach()) - float(g["total"])) < 1e-5 * abs(float(g["total"]))
    assert abs(float(crit.loss_dict["reg_loss"]) - float(g["reg"])) < 1e-5 * abs(float(g["reg"]))
    assert abs(float(crit.loss_dict["conf_loss"]) - float(g["conf"])) < 1e-5 * abs(float(g["conf"]))
    assert rel_max_err(p.grad.cpu() / 3.0, g["d_psm"]) < 1e-5
    assert rel_max_err(r.grad.cpu() / 3.0, g["d_rm"]) < 1e-5


def test_detector_training_precision_and_errors():
    """.train() without set_return_features(): a detector in the default precision ('split') returns its heads from the training
    forward; one built with 'f32' or 'f16' is refused (the training layers run split products), its feature path still trains; host
    tensors are refused."""
    import hmvit_amd
    from oracle import pointpillar_oracle as PO
    g = load_golden("g7_pointpillar.npz")
    nx, ny = [int(v) for v in g["grid"]]
    args = PO.make_args(nx, ny)
    sd = PO.random_state_dict(args, g["seed_weights"])
    vf, vc, vn = PO.synthetic_pillars(int(g["n_agents"]), int(g["n_per_agent"]), nx, ny, args, int(g["seed_pillars"]))
    batch = {"processed_lidar": {"voxel_features": vf.cuda(), "voxel_coords": vc.cuda(), "voxel_num_points": vn.cuda()}}
    net = hmvit_amd.PointPillar(args)
    net.load_state_dict(sd, strict=True)
    net = net.cuda()
    with torch.no_grad():
        ev = net.eval()(batch)
    tr = net.train()(batch)
    assert set(tr) == {"psm", "rm"} and tr["psm"].shape == ev["psm"].shape and tr["rm"].shape == ev["rm"].shape
    assert tr["psm"].requires_grad and bool(torch.isfinite(tr["psm"]).all()) and bool(torch.isfinite(tr["rm"]).all())
    with pytest.raises(RuntimeError, match="GPU only"):
        net({"processed_lidar": {"voxel_features": vf, "voxel_coords": vc, "voxel_num_points": vn}})
    for precision in ("f32", "f16"):
        other = hmvit_amd.PointPillar(args, precision=precision)
        other.load_state_dict(sd, strict=True)
        other = other.cuda().train()
        with pytest.raises(NotImplementedError, match="precision 'split'"):
            other(batch)
        other.set_return_features()
        assert other(batch).requires_grad


def _detector_reference(net, vf, vc, vn, n_agents):
    """PointPillar.forward of the standalone detector from the module's own torch layers (pillar_vfe.py:105-146,31-53,
    point_pillar_scatter.py:14-47, base_bev_backbone.py:89-122, downsample_conv.py:32-51, point_pillar.py:56-62)."""
    from hmvit_amd.encoder_train import pfn_features
    nx, ny, _ = [int(v) for v in net.scatter_cfg["grid_size"]]
    pfn = net.pillar_vfe.pfn_layers[0]
    feats = pfn_features(vf, vc.long(), vn, net.args["voxel_size"], net.args["lidar_range"])
    h = torch.relu(pfn.norm(pfn.linear(feats).permute(0, 2, 1)).permute(0, 2, 1)).max(dim=1)[0]
    canvas = torch.zeros(n_agents, 64, ny * nx, dtype=h.dtype)
    for b in range(n_agents):
        m = vc[:, 0] == b
        canvas[b][:, (vc[m, 2] * nx + vc[m, 3]).long()] = h[m].t()
    x = canvas.view(n_agents, 64, ny, nx)
    ups = []
    for blk, de in zip(net.backbone.blocks, net.backbone.deblocks):
        x = blk(x)
        ups.append(de(x))
    x = torch.cat(ups, dim=1)
    for dc in net.shrink_conv.layers:
        x = dc.double_conv(x)
    return {"psm": net.cls_head(x), "rm": net.reg_head(x)}


def test_detector_training_forward_and_backward_match_torch():
    """PointPillar in .train() without set_return_features(): psm / rm and every parameter gradient (heads included) against a
    float64 torch copy, held to the yardstick of test_hip_trainer.py::test_pointpillar_training_matches_torch_modules; running
    statistics updated; .eval() afterwards on the folded kernels."""
    import hmvit_amd
    from oracle import pointpillar_oracle as PO
    args = PO.make_args(64, 48, small=True)
    sd = PO.random_state_dict(args, seed=3)
    vf, vc, vn = PO.synthetic_pillars(2, 400, 64, 48, args, seed=4)
    net = hmvit_amd.PointPillar(args, precision="split")
    net.load_state_dict(sd, strict=True)
    ref = copy.deepcopy(net).double().train()
    ref32 = copy.deepcopy(net).float().train()
    net = net.cuda().train()
    batch = {"processed_lidar": {"voxel_features": vf.cuda(), "voxel_coords": vc.cuda(), "voxel_num_points": vn.cuda()}, "n_agents": 2}
    y = net(batch)
    y_ref = _detector_reference(ref, vf.double(), vc, vn, 2)
    y_32 = _detector_reference(ref32, vf.float(), vc, vn, 2)
    err = lambda a, b: float((a.cpu().double() - b.cpu().double()).abs().max() / b.abs().max().clamp_min(1e-12))
    gen = torch.Generator().manual_seed(1)
    gs = {k: torch.randn(y_ref[k].shape, generator=gen) for k in ("psm", "rm")}
    for k in ("psm", "rm"):
        assert y[k].shape == y_ref[k].shape and y[k].dtype == torch.float32 and y[k].is_contiguous()
        assert err(y[k].detach(), y_ref[k].detach()) < 1e-4, k
    sum(((y[k] * gs[k].cuda()).sum() for k in gs)).backward()
    sum(((y_ref[k] * gs[k].double()).sum() for k in gs)).backward()
    sum(((y_32[k] * gs[k]).sum() for k in gs)).backward()

    gmax = max(float(q.grad.abs().max()) for q in ref.parameters() if q.grad is not None)

    def rel(a, b, floor):
        a, b = a.cpu().double(), b.cpu().double()
        d = (a - b).abs() / max(float(b.abs().max()), floor, 1e-12)
        return float(d.pow(2).mean().sqrt()), float((d > 4e-3).double().sum()) / max(2.0, 1e-3 * d.numel())
    worst, used = {}, 0
    for (k, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
        assert q.grad is not None and p.grad is not None, k                  # every parameter is on the tape, heads included
        used += 1
        worst[k] = rel(p.grad, q.grad, 1e-3 * gmax)
    yard = {k: rel(p.grad, q.grad, 1e-3 * gmax)[0] for (k, p), (_, q) in zip(ref32.named_parameters(), ref.named_parameters())}
    bad = {k: (v, yard[k]) for k, v in worst.items() if not (v[0] < max(3 * yard[k], 2e-4) and v[1] <= 1.0)}
    assert not bad, bad
    assert used == len(list(net.parameters())) and {"cls_head.weight", "cls_head.bias", "reg_head.weight", "reg_head.bias"} <= set(worst)
    for (k, a), (_, b) in zip(net.named_buffers(), ref.named_buffers()):
        if a.is_floating_point():
            assert err(a, b) < 1e-4, k
    for key in ("backbone.blocks.0.2.num_batches_tracked", "pillar_vfe.pfn_layers.0.norm.num_batches_tracked"):
        assert int(net.state_dict()[key]) == int(sd[key]) + 1, key              # one training forward
    net.eval(); ref.eval()
    with torch.no_grad():
        ye = net(batch)
        ye_ref = _detector_reference(ref, vf.double(), vc, vn, 2)
    for k in ("psm", "rm"):
        assert err(ye[k], ye_ref[k]) < 2e-4, k


def _json_line(text):
    return json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])


def test_stage1_trains_hands_over_and_replays_late(tmp_path, capsys):
    import hmvit_amd
    from hmvit_amd import replay as R
    from hmvit_amd import trainer as T
    s1 = tmp_path / "stage1"
    # ---- stage 1: the standalone detector on single-agent samples, the fused loss ----
    T.main(["--stage", "lidar_backbone", "--small", "--grid", "64", "64", "--agents", "3", "--epochs", "2", "--frames", "8",
            "--batch", "4", "--val_frames", "4", "--model_dir", str(s1)])
    res = _json_line(capsys.readouterr().out)
    assert res["stage"] == "lidar_backbone" and res["steps"] == 3 and len(res["epoch_loss"]) == 2
    assert all(math.isfinite(v) for v in res["epoch_loss"] + res["val_loss"])
    assert res["epoch_loss"][1] < res["epoch_loss"][0], res
    assert sorted(p.name for p in s1.iterdir()) == ["net_epoch1.pth", "net_epoch2.pth"]
    saved = torch.load(s1 / "net_epoch2.pth", map_location="cpu")
    cfg = R.lidar_model_config(64, 64, max_cav=3, small=True)
    assert list(saved) == list(hmvit_amd.PointPillar(cfg["lidar"]).state_dict())

    # ---- stage 2: the checkpoint into model.lidar_encoder, frozen; the fusion trains ----
    class Stage2:
        stage, grid, agents, small, precision, seed, frames, train_lidar_backbone = "hetero", [128, 96], 3, True, "f32", 0, 2, False
        val_frames, camera_ratio, ego_mode, camera_image, train_camera_backbone = 0, 0.0, "mixed", 64, False
        lidar_backbone_dir = str(s1)
    _, model, pre, _, ds, _ = T.build(Stage2)
    enc = model.lidar_encoder.state_dict()
    assert all(torch.equal(enc[k], saved[k]) for k in saved)
    model = model.cuda()
    hypes = T.default_hypes(1)
    hypes["loss"]["fused"] = True                                    # --fused_loss
    out = T.train(model, ds, pre, hypes)
    assert math.isfinite(out["epoch_loss"][0])
    assert all(p.grad is None for p in model.lidar_encoder.parameters())
    after = model.lidar_encoder.state_dict()
    assert all(torch.equal(after[k].cpu(), saved[k]) for k in saved)
    assert model.fusion_net.mlp_head.net[1][0].weight.grad is not None

    # ---- late-fusion replay of the stage-1 checkpoint ----
    R.main(["--late", "--small", "--checkpoint", str(s1 / "net_epoch2.pth"), "--scenes", "2", "--agents", "3", "--grid", "64", "64",
            "--precision", "f32"])
    rep = _json_line(capsys.readouterr().out)
    assert rep["fusion"] == "late" and rep["frames"] == 2
    assert {"AP@0.3", "AP@0.5", "AP@0.7"} <= set(rep)


def test_stage1_step_at_the_shipped_size(capsys):
    """point_pillar_late_fusion.yaml's size: 512 x 512 pillars, layer_nums [3, 5, 8], batch 8 single-agent samples; two steps
    (the second one timed)."""
    from hmvit_amd import trainer as T
    torch.cuda.reset_peak_memory_stats()
    T.main(["--stage", "lidar_backbone", "--grid", "512", "512", "--epochs", "1", "--frames", "16", "--batch", "8",
            "--val_frames", "0"])
    res = _json_line(capsys.readouterr().out)
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    assert res["steps"] == 1 and math.isfinite(res["epoch_loss"][0])
    with capsys.disabled():
        print(f"\nstage 1 at 512 x 512, batch 8: {res['ms_per_step']:.1f} ms per step, loss {res['epoch_loss'][0]:.4f}, "
              f"peak {peak:.2f} GiB")
