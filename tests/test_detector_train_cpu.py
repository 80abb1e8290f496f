"""CPU tests of the LiDAR backbone pretraining's host side (hm-vit_amd/trainer.py): the single-agent late-fusion samples of stage 1
(one seeded-random agent per frame, boxes in that agent's frame), the loss selection, the CLI and the stage-1 -> stage-2 hand-over
of the encoder's weights by key."""
import math
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)


class _Stage1:
    stage, grid, agents, small, seed, frames, batch, val_frames = "lidar_backbone", [64, 64], 3, True, 0, 6, 4, 0


def _dataset(seed=7, n=12):
    import hmvit_amd  # noqa: F401
    from hmvit_amd import replay as R
    from hmvit_amd import trainer as T
    from hmvit_amd.postprocess import VoxelPostprocessor
    cfg = R.lidar_model_config(96, 96, max_cav=3, small=True)
    post = VoxelPostprocessor(R.postprocess_params(cfg), train=True)
    return cfg, T.LateFusionTrainDataset(cfg, n, post, n_agents=3, seed=seed), R.SyntheticReplayDataset(cfg, n, n_agents=3, seed=seed)


def _wrap(a):
    return (np.asarray(a) + math.pi) % (2 * math.pi) - math.pi


def test_cav_frame_boxes_inverts_the_pose():
    from hmvit_amd import synthetic as S
    from hmvit_amd import trainer as T
    rs = np.random.RandomState(0)
    boxes = np.concatenate([rs.uniform(-30, 30, (20, 2)), rs.uniform(-1.5, -0.5, (20, 1)), np.tile([[1.56, 1.6, 3.9]], (20, 1)),
                            rs.uniform(-math.pi, math.pi, (20, 1))], 1).astype(np.float32)
    pose = S.rigid(0.7, 12.0, -5.0).numpy()
    local = T.cav_frame_boxes(boxes, pose)
    back = local[:, :3].astype(np.float64) @ pose[:3, :3].T + pose[:3, 3]
    assert np.abs(back - boxes[:, :3]).max() < 1e-4
    assert np.abs(_wrap(local[:, 6] + 0.7 - boxes[:, 6])).max() < 1e-5
    assert np.all(local[:, 6] >= -math.pi) and np.all(local[:, 6] < math.pi)
    assert np.array_equal(local[:, 3:6], boxes[:, 3:6])


def test_late_fusion_sample_is_one_agent_in_its_own_frame():
    cfg, ds, frames = _dataset()
    rng = cfg["lidar"]["lidar_range"]
    n_pos = 0
    for i in range(len(ds)):
        s, f = ds[i], frames[i]
        cav = s["cav"]
        assert 0 <= cav < 3
        assert np.array_equal(s["cloud"], f["clouds"][cav])               # that agent's own cloud, nothing else
        pose = f["lidar_poses"][cav]
        assert np.array_equal(s["lidar_pose"], pose)
        k = len(s["object_ids"])
        assert s["object_bbx_mask"].sum() == k and not s["object_bbx_center"][k:].any()
        # the inverse transform (agent -> ego) of the sample's boxes recovers the ego-frame boxes
        local = s["object_bbx_center"][:k].astype(np.float64)
        ego = f["object_bbx_center_valid"][s["object_ids"]]
        assert np.abs(local[:, :3] @ pose[:3, :3].T + pose[:3, 3] - ego[:, :3]).max() < 1e-4
        assert np.abs(_wrap(local[:, 6] + math.atan2(pose[1, 0], pose[0, 0]) - ego[:, 6])).max() < 1e-5
        # kept: exactly the boxes whose centre lies inside the agent's range
        every = f["object_bbx_center_valid"]
        allb = (np.linalg.inv(pose) @ np.c_[every[:, :3], np.ones(len(every))].T).T
        inside = np.nonzero((allb[:, 0] > rng[0]) & (allb[:, 0] < rng[3]) & (allb[:, 1] > rng[1]) & (allb[:, 1] < rng[4]))[0]
        assert np.array_equal(inside, s["object_ids"])
        lab = s["label_dict"]
        assert lab["pos_equal_one"].shape == (*ds.anchors.shape[:2], 2) and lab["targets"].shape == (*ds.anchors.shape[:2], 14)
        n_pos += int(lab["pos_equal_one"].sum())
    assert n_pos > 0


def test_late_fusion_agent_choice_is_seeded():
    _, a, _ = _dataset(seed=7, n=16)
    _, b, _ = _dataset(seed=7, n=16)
    _, c, _ = _dataset(seed=8, n=16)
    ca = [a.pick_cav(i) for i in range(16)]
    assert ca == [b.pick_cav(i) for i in range(16)]
    assert len(set(ca)) > 1                                               # not always the ego
    assert ca != [c.pick_cav(i) for i in range(16)]
    sa, sb = a[5], b[5]
    assert sa["cav"] == sb["cav"] and np.array_equal(sa["cloud"], sb["cloud"])
    assert np.array_equal(sa["label_dict"]["targets"], sb["label_dict"]["targets"])


def test_batches_group_consecutive_samples():
    from hmvit_amd import trainer as T
    _, ds, _ = _dataset(n=10)
    bt = T.Batched(ds, 4)
    assert len(bt) == 3
    assert [s["cav"] for s in bt[1]] == [ds.pick_cav(i) for i in range(4, 8)]
    assert len(bt[2]) == 2


def test_fused_loss_is_opt_in_and_has_no_cpu_fallback():
    import hmvit_amd
    from hmvit_amd import trainer as T
    hypes = T.default_hypes(1)
    assert type(T.create_loss(hypes)) is hmvit_amd.PointPillarLoss
    hypes["loss"]["fused"] = True
    crit = T.create_loss(hypes)
    assert isinstance(crit, hmvit_amd.FusedPointPillarLoss)
    assert (crit.cls_weight, crit.reg_coe, crit.alpha, crit.gamma, crit.beta) == (1.0, 2.0, 0.25, 2.0, 1.0 / 9.0)
    from make_goldens_inputs import loss_inputs
    psm, rm, tgt = loss_inputs()
    with pytest.raises(RuntimeError, match="GPU only"):
        crit({"psm": psm, "rm": rm}, tgt)


def test_stage1_model_keys_match_the_lidar_encoder_and_hand_over(tmp_path):
    """The stage-1 checkpoint is the standalone PointPillar's state_dict; --lidar_backbone_dir loads it into model.lidar_encoder
    (same keys, heads included) before the encoder is frozen."""
    from hmvit_amd import trainer as T
    cfg, model, pre, post, ds, val = T.build(_Stage1)
    assert type(model).__name__ == "PointPillar" and not model.return_features
    assert len(ds) == 2 and val is None
    assert {k.split(".")[0] for k in model.state_dict()} == {"pillar_vfe", "backbone", "shrink_conv", "cls_head", "reg_head"}
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.125)                                               # distinguishable from a fresh initialisation
    path = T.save_checkpoint(model, str(tmp_path), 1)
    assert path.endswith("net_epoch2.pth")

    class Stage2:
        stage, grid, agents, small, precision, seed, frames, train_lidar_backbone = "hetero", [128, 96], 3, True, "f32", 0, 2, False
        val_frames, camera_ratio, ego_mode, camera_image, train_camera_backbone = 0, 0.0, "mixed", 64, False
        lidar_backbone_dir = str(tmp_path)
    _, hetero, _, _, _, _ = T.build(Stage2)
    enc = hetero.lidar_encoder.state_dict()
    saved = torch.load(path, map_location="cpu")
    assert list(enc) == list(saved)
    assert all(torch.equal(enc[k], saved[k]) for k in saved)
    assert hetero._fix_lidar_backbone

    class Missing(Stage2):
        lidar_backbone_dir = str(tmp_path / "nothing-here")
    with pytest.raises(FileNotFoundError):
        T.build(Missing)
