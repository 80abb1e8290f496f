"""GPU tests of the standalone FAX camera detector (``FaxCameraEncoder`` = ``FaxFusedTransformer`` without
``set_return_features()``): heads against the oracle composition in eval mode and under float64 autograd in train mode, the camera
stage of the trainer and its hand-over to stage 2, mixed late fusion and no fusion in the replay driver, and one stage-1 step at the
size of ``fax_late_fusion.yaml``."""
import json
import math
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_max_err
from oracle import camera_oracle as CAM
from oracle import cvt_oracle as CO
from oracle import fax_oracle as FO

pytestmark = pytest.mark.gpu


def _detector(cfg, precision, seed, features=False):
    import hmvit_amd
    torch.manual_seed(seed)
    net = hmvit_amd.FaxCameraEncoder(cfg, precision=precision)
    with torch.no_grad():                                   # non-trivial BatchNorm statistics / LayerNorm affines
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.2); m.running_var.uniform_(0.6, 1.4); m.weight.normal_(1, 0.1); m.bias.normal_(0, 0.1)
            if isinstance(m, torch.nn.LayerNorm):
                m.weight.normal_(1, 0.1); m.bias.normal_(0, 0.1)
    if features:
        net.set_return_features()
    return net.cuda().eval()


def _heads(feat, sd):
    return {"psm": F.conv2d(feat.double(), sd["cls_head.weight"].double(), sd["cls_head.bias"].double()),
            "rm": F.conv2d(feat.double(), sd["reg_head.weight"].double(), sd["reg_head.bias"].double())}


@pytest.mark.parametrize("precision,tol", [("f32", 3e-4), ("split", 3e-4), ("f16", 1e-2)])
def test_camera_detector_heads_vs_oracle(precision, tol):
    cfg = FO.make_camera_config(image=64)
    net = _detector(cfg, precision, seed=9)
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    batch = CAM.synthetic_batch(2, CAM.make_config(image=64), seed=10)
    keys = set(batch)
    feat = FO.fax_camera_encoder(batch, sd, cfg)
    ref = _heads(feat, sd)
    gpu = {k: v.cuda() for k, v in batch.items()}
    with torch.no_grad():
        out = net(gpu)
    assert set(out) == {"psm", "rm"} and set(gpu) == keys and gpu["camera"].dim() == 5      # the batch dict is left alone
    assert out["psm"].shape == (2, 2, 32, 32) and out["rm"].shape == (2, 14, 32, 32)
    for k in ("psm", "rm"):
        assert out[k].dtype == torch.float32 and out[k].is_contiguous()
        err = rel_max_err(out[k].cpu(), ref[k])
        print(f"\ncamera detector [{precision}] {k}: rel-max {err:.1e}")
        assert err < tol, (k, err)
    twin = _detector(cfg, precision, seed=9, features=True)                 # the camera-slot contract is unchanged
    with torch.no_grad():
        y = twin(gpu).cpu()
    assert y.shape == feat.shape == (2, 256, 32, 32)
    assert rel_max_err(y, feat) < tol


def _labels(B, seed):
    from hmvit_amd import replay as R
    from hmvit_amd.postprocess import VoxelPostprocessor
    post = VoxelPostprocessor(R.postprocess_params(R.lidar_model_config(128, 128)), train=True)
    anchors = post.generate_anchor_box()
    assert anchors.shape[:2] == (32, 32)
    rs = np.random.RandomState(seed)
    labels = []
    for _ in range(B):
        center = np.zeros((8, 7), np.float32)
        mask = np.zeros(8, np.float32)
        for i in range(4):
            center[i] = [rs.uniform(-20, 20), rs.uniform(-20, 20), -1.0, 1.56, 1.6, 3.9, rs.uniform(-math.pi, math.pi)]
            mask[i] = 1
        labels.append(post.generate_label(gt_box_center=center, anchors=anchors, mask=mask))
    return {k: v.float() for k, v in VoxelPostprocessor.collate_batch(labels).items()}


def test_camera_detector_training_matches_float64_autograd():
    """``.train()`` without set_return_features(): psm / rm and the gradient of every parameter (heads included) under
    FusedPointPillarLoss, against float64 torch.autograd through the oracle composition (batch-statistics BatchNorm) with
    PointPillarLoss; the bounds of test_hip_camera_train.py::test_fax_camera_encoder_training_matches_float64_autograd."""
    import hmvit_amd
    from hmvit_amd import FusedPointPillarLoss, PointPillarLoss
    cfg = FO.make_camera_config(image=64)
    cfg["fax"]["self_attn"]["dropout"] = 0.0                 # the one Dropout of the branch: off, so that both sides are deterministic
    net = _detector(cfg, "f32", seed=9)
    csd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    net.train()
    batch = CAM.synthetic_batch(2, CAM.make_config(image=64), seed=10)
    tgt = _labels(2, seed=3)
    ref_sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in csd.items()}
    ref_sd = {k: (v.requires_grad_(True) if v.is_floating_point() and "running_" not in k else v) for k, v in ref_sd.items()}
    with CO.batch_statistics():
        feat = FO.fax_camera_encoder({k: v.double() for k, v in batch.items()}, ref_sd, cfg)
    ref = _heads(feat, ref_sd)
    crit_ref = PointPillarLoss({"cls_weight": 1.0, "reg": 2.0})
    loss_ref = crit_ref(ref, {k: v.double() for k, v in tgt.items()})
    loss_ref.backward()

    out = net({k: v.cuda() for k, v in batch.items()})
    assert set(out) == {"psm", "rm"} and out["psm"].requires_grad
    for k in ("psm", "rm"):
        err = rel_max_err(out[k].detach().cpu(), ref[k].detach())
        print(f"\ncamera detector (training forward) {k}: rel-max {err:.1e} against float64")
        assert err < 1e-4, (k, err)
    crit = FusedPointPillarLoss({"cls_weight": 1.0, "reg": 2.0})
    loss = crit(out, {k: v.cuda() for k, v in tgt.items()})
    assert abs(float(loss.detach()) - float(loss_ref.detach())) < 1e-3 * abs(float(loss_ref.detach()))
    loss.backward()
    err, num, den = {}, 0.0, 0.0
    nmax = max(float(v.grad.norm()) for v in ref_sd.values() if getattr(v, "grad", None) is not None)
    for name, p in net.named_parameters():
        assert p.grad is not None, name                      # every parameter is on the tape, heads included
        r = ref_sd[name]
        assert r.grad is not None, name
        d = (p.grad.cpu().double() - r.grad).norm()
        num, den = num + float(d) ** 2, den + float(r.grad.norm()) ** 2
        err[name] = float(d / r.grad.norm().clamp_min(1e-6 * nmax))
    vals = sorted(err.values())
    top = sorted(err.items(), key=lambda kv: -kv[1])[:5]
    total = (num / den) ** 0.5
    print(f"\ncamera detector: {len(err)} parameter gradients vs float64 autograd: all together {total:.1e}; median "
          f"{vals[len(vals) // 2]:.1e}, worst", [(k, f"{v:.1e}") for k, v in top])
    assert {"cls_head.weight", "cls_head.bias", "reg_head.weight", "reg_head.bias"} <= set(err)
    assert max(err[k] for k in ("cls_head.weight", "cls_head.bias", "reg_head.weight", "reg_head.bias")) < 2e-2
    assert total < 2e-2 and vals[len(vals) // 2] < 2e-2 and vals[-1] < 1e-1, (total, top)


def _json_line(text):
    return json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])


def test_camera_stage_trains_hands_over_and_replays_mixed_late(tmp_path, capsys):
    import hmvit_amd
    from hmvit_amd import replay as R
    from hmvit_amd import synthetic as S
    from hmvit_amd import trainer as T
    s1c, s1l = tmp_path / "stage1_camera", tmp_path / "stage1_lidar"
    # ---- camera stage 1: the FAX detector on single camera-agent samples, the fused loss, batch 3 by default ----
    T.main(["--stage", "camera_backbone", "--grid", "128", "128", "--camera_image", "64", "--agents", "3", "--epochs", "2",
            "--frames", "6", "--val_frames", "3", "--model_dir", str(s1c)])
    res = _json_line(capsys.readouterr().out)
    assert res["stage"] == "camera_backbone" and res["batch"] == 3 and res["steps"] == 3 and len(res["epoch_loss"]) == 2
    assert all(math.isfinite(v) for v in res["epoch_loss"] + res["val_loss"])
    assert sorted(p.name for p in s1c.iterdir()) == ["net_epoch1.pth", "net_epoch2.pth"]
    saved = torch.load(s1c / "net_epoch2.pth", map_location="cpu")
    assert list(saved) == list(hmvit_amd.FaxCameraEncoder(S.fax_camera_config(128, 128, 64)).state_dict())

    # ---- stage 2: the checkpoint into the FAX camera slot, frozen ----
    class Stage2:
        stage, grid, agents, small, precision, seed, frames, train_lidar_backbone = "hetero", [128, 128], 3, True, "f32", 0, 2, False
        val_frames, camera_ratio, ego_mode, camera_image, train_camera_backbone = 0, 0.5, "camera", 64, False
        camera_encoder, camera_backbone_dir = "fax", str(s1c)
    _, model, pre, _, ds, _ = T.build(Stage2)
    assert type(model.camera_encoder) is hmvit_amd.FaxCameraEncoder
    slot = model.camera_encoder.state_dict()
    assert list(slot) == list(saved) and all(torch.equal(slot[k], saved[k]) for k in saved)
    model = model.cuda()
    out = T.train(model, ds, pre, T.default_hypes(1))
    assert math.isfinite(out["epoch_loss"][0])
    assert all(p.grad is None for p in model.camera_encoder.parameters())
    after = model.camera_encoder.state_dict()
    assert all(torch.equal(after[k].cpu(), saved[k]) for k in saved)
    assert model.fusion_net.mlp_head.net[0][0].weight.grad is not None      # the camera ego's typed head trained

    # ---- mixed late fusion replay: LiDAR stage-1 detector + camera stage-1 detector ----
    T.main(["--stage", "lidar_backbone", "--small", "--grid", "128", "128", "--agents", "3", "--epochs", "1", "--frames", "4",
            "--batch", "4", "--val_frames", "0", "--model_dir", str(s1l)])
    capsys.readouterr()
    R.main(["--late", "--camera_ratio", "0.5", "--camera_checkpoint", str(s1c / "net_epoch2.pth"), "--checkpoint",
            str(s1l / "net_epoch1.pth"), "--small", "--scenes", "2", "--agents", "3", "--grid", "128", "128", "--precision", "f32"])
    rep = _json_line(capsys.readouterr().out)
    assert rep["fusion"] == "late" and rep["frames"] == 2 and rep["camera_ratio"] == 0.5 and rep["ego_mode"] == "mixed"
    assert rep["camera_agents"] > 0
    assert {"AP@0.3", "AP@0.5", "AP@0.7"} <= set(rep)
    with capsys.disabled():
        print(f"\nmixed late fusion replay: {json.dumps(rep)}")


def test_camera_stage1_overfits_one_batch():
    import argparse
    from hmvit_amd import trainer as T
    from hmvit_amd.train import FusedPointPillarLoss, make_optimizer
    args = argparse.Namespace(stage="camera_backbone", grid=[128, 128], camera_image=64, agents=3, seed=0, frames=3, batch=3,
                              val_frames=0, small=False)
    _, model, _, _, ds, _ = T.build(args)
    model = model.cuda()
    batch = T.to_late_camera_batch(ds[0], None, "cuda")
    crit = FusedPointPillarLoss({"cls_weight": 1.0, "reg": 2.0})
    opt = make_optimizer(model.parameters(), {"lr": 2e-4})
    losses = []
    for _ in range(6):
        model.train()
        opt.zero_grad()
        loss = crit(model(batch), batch["label_dict"])
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("\ncamera stage 1, one batch:", [f"{v:.4f}" for v in losses])
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]


def _late_setup(ego_mode, seed=7):
    import hmvit_amd
    from hmvit_amd import replay as R
    from hmvit_amd import synthetic as S
    cfg = R.lidar_model_config(128, 128, max_cav=3, small=True)
    torch.manual_seed(5)
    lidar = hmvit_amd.PointPillar(cfg["lidar"], precision="f32")
    camera = hmvit_amd.FaxCameraEncoder(S.fax_camera_config(128, 128, 64), precision="f32")
    with torch.no_grad():                                   # anchor-like boxes; the logits keep their spread (distinct scores)
        for m in (lidar, camera):
            m.reg_head.weight.mul_(0.02)
            m.reg_head.bias.zero_()
    lidar, camera = lidar.cuda().eval(), camera.cuda().eval()
    pre = hmvit_amd.SpVoxelPreprocessor(R.preprocess_params(cfg), train=False)
    post = hmvit_amd.VoxelPostprocessor(R.postprocess_params(cfg), train=False)
    ds = R.SyntheticReplayDataset(cfg, 2, n_agents=3, seed=seed, camera_ratio=0.5, ego_mode=ego_mode, camera_image=64)
    return lidar, camera, pre, post, ds


def _alone(frame, a, lidar, camera, pre):
    """Agent a's detector on that agent alone (batch 1)."""
    if int(frame["mode"][0, a]) == 1:
        return lidar({"processed_lidar": pre.collate_batch([pre.preprocess(frame["clouds"][a])]), "n_agents": 1})
    return camera({k: frame[k][a:a + 1].cuda() for k in ("camera", "intrinsic", "extrinsic")})


def _threshold(heads, top=150):
    """A score threshold in a gap of the scores near the top `top`, so that last-bit differences cannot move a box across it."""
    s = torch.sigmoid(torch.cat([h["psm"].reshape(-1) for h in heads.values()]).double()).sort(descending=True).values.cpu()
    for k in range(top, min(len(s), 10 * top)):
        if float(s[k - 1] - s[k]) > 1e-6:
            return float((s[k - 1] + s[k]) / 2)
    raise AssertionError("no gap in the scores")


def _same_boxes(a, b):
    (ba, sa), (bb, sb) = a, b
    assert ba is not None and bb is not None and len(ba) == len(bb) > 0
    scale = max(1.0, float(bb.abs().max()))
    assert float((ba - bb).abs().max()) <= 1e-6 * scale
    assert float((sa - sb).abs().max()) <= 1e-6


def test_mixed_late_fusion_is_the_composition_of_single_agent_detectors():
    from hmvit_amd import replay as R
    lidar, camera, pre, post, ds = _late_setup("camera")
    frame = ds[1]
    modes = [int(v) for v in frame["mode"][0, :3]]
    assert 0 in modes and 1 in modes, modes
    with torch.no_grad():
        heads = {a: _alone(frame, a, lidar, camera, pre) for a in range(3)}
    post.params["target_args"]["score_threshold"] = _threshold(heads)
    poses = torch.from_numpy(frame["lidar_poses"]).float()
    anchors = torch.from_numpy(post.generate_anchor_box())
    ref = post.post_process({a: {"anchor_box": anchors, "transformation_matrix": poses[a]} for a in range(3)},
                            {a: {"psm": h["psm"], "rm": h["rm"]} for a, h in heads.items()})
    got = []

    class One:
        def __len__(self):
            return 1

        def __getitem__(self, i):
            return frame
    with torch.no_grad():
        res = R.inference(lidar, One(), pre, post, calibrate_top=None, late=True, camera_model=camera, outputs=got)
    assert res["camera_agents"] == modes.count(0)
    _same_boxes(got[0], ref)


@pytest.mark.parametrize("ego_mode", ["camera", "lidar"])
def test_nofusion_runs_only_the_ego_detector(ego_mode, monkeypatch):
    from hmvit_amd import replay as R
    lidar, camera, pre, post, ds = _late_setup(ego_mode)
    frame = ds[1]
    assert int(frame["mode"][0, 0]) == (0 if ego_mode == "camera" else 1)
    with torch.no_grad():
        ego = _alone(frame, 0, lidar, camera, pre)
    post.params["target_args"]["score_threshold"] = _threshold({0: ego}, top=60)
    anchors = torch.from_numpy(post.generate_anchor_box())
    ref = post.post_process({0: {"anchor_box": anchors, "transformation_matrix": torch.eye(4)}}, {0: ego})

    def refuse(*a, **k):
        raise AssertionError("the other detector was called")
    monkeypatch.setattr(lidar if ego_mode == "camera" else camera, "forward", refuse)

    class One:
        def __len__(self):
            return 1

        def __getitem__(self, i):
            return frame
    got = []
    with torch.no_grad():
        R.inference(lidar, One(), pre, post, calibrate_top=None, camera_model=camera, nofusion=True, outputs=got)
    _same_boxes(got[0], ref)


def test_camera_stage1_step_at_the_shipped_size():
    """fax_late_fusion.yaml's model block: ResNet-18 on 4 cameras of 512 x 512, BEV 256 over 100 m, q windows [[16, 16], [16, 16],
    [32, 32]], feature windows [[8, 8], [8, 8], [16, 16]], self-attention window 32, batch 3, head grid 128 x 128 x 2.  Two training
    steps (the second one timed), then one eval forward."""
    import hmvit_amd
    from hmvit_amd import replay as R
    from hmvit_amd import synthetic as S
    from hmvit_amd import trainer as T
    from hmvit_amd.postprocess import VoxelPostprocessor
    from hmvit_amd.train import FusedPointPillarLoss, make_optimizer
    ccfg = S.fax_camera_config(512, 512, 512, meters=100.0)
    cfg = R.lidar_model_config(512, 512, max_cav=3)
    post = VoxelPostprocessor(R.postprocess_params(cfg), train=True)
    ds = T.LateFusionTrainDataset(cfg, 3, post, n_agents=3, seed=7, modality="camera", camera_image=512)
    batch = T.to_late_camera_batch([ds[i] for i in range(3)], None, "cuda")
    torch.manual_seed(0)
    model = hmvit_amd.FaxFusedTransformer(ccfg).cuda()
    crit = FusedPointPillarLoss({"cls_weight": 1.0, "reg": 2.0})
    opt = make_optimizer(model.parameters(), {"lr": 2e-4})
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    for step in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.train()
        opt.zero_grad()
        out = model(batch)
        loss = crit(out, batch["label_dict"])
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0)
    assert out["psm"].shape == (3, 2, 128, 128) and out["rm"].shape == (3, 14, 128, 128)
    assert math.isfinite(float(loss.detach()))
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    model.eval()
    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev = model({k: batch[k] for k in ("camera", "intrinsic", "extrinsic")})
        torch.cuda.synchronize()
        ms_eval = 1e3 * (time.perf_counter() - t0)
    assert ev["psm"].shape == (3, 2, 128, 128) and bool(torch.isfinite(ev["psm"]).all()) and bool(torch.isfinite(ev["rm"]).all())
    print(f"\ncamera stage 1 at 4 x 512 x 512 images, BEV 256, batch 3: {ms:.1f} ms per training step, peak {peak:.2f} GiB; "
          f"eval forward {ms_eval:.1f} ms (first call, weight preparation included), loss {float(loss.detach()):.4f}")
