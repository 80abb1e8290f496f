"""CPU tests of the camera half of the two-stage recipe (hm-vit_amd/trainer.py, replay.py, synthetic.py): the single camera-agent
samples of ``--stage camera_backbone``, the FAX detector config helper, the stage-1 -> stage-2 hand-over of the camera detector's
weights by key, the argument checks that run before any device work, and the replay frames without camera agents."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN


def _camera_dataset(seed=7, n=10, image=32):
    import hmvit_amd  # noqa: F401
    from hmvit_amd import replay as R
    from hmvit_amd import trainer as T
    from hmvit_amd.postprocess import VoxelPostprocessor
    cfg = R.lidar_model_config(96, 96, max_cav=3, small=True)
    post = VoxelPostprocessor(R.postprocess_params(cfg), train=True)
    ds = T.LateFusionTrainDataset(cfg, n, post, n_agents=3, seed=seed, modality="camera", camera_image=image)
    frames = R.SyntheticReplayDataset(cfg, n, n_agents=3, seed=seed, camera_ratio=1.0, ego_mode="camera", camera_image=image)
    return cfg, ds, frames


def _wrap(a):
    return (np.asarray(a) + math.pi) % (2 * math.pi) - math.pi


def test_camera_late_fusion_sample_is_one_agent_with_its_cameras():
    cfg, ds, frames = _camera_dataset()
    rng = cfg["lidar"]["lidar_range"]
    n_pos = 0
    for i in range(len(ds)):
        s, f = ds[i], frames[i]
        cav = s["cav"]
        assert 0 <= cav < 3
        assert "cloud" not in s                                            # a camera sample: no point cloud
        assert torch.equal(f["mode"][0, :3], torch.zeros(3, dtype=torch.float64))   # ratio 1, ego camera: every agent a camera agent
        for k, shape in (("camera", (4, 32, 32, 3)), ("intrinsic", (4, 3, 3)), ("extrinsic", (4, 4, 4))):
            assert tuple(s[k].shape) == shape, k
            assert torch.equal(s[k], f[k][cav]), k                         # that agent's own tensors, nothing else
        pose = f["lidar_poses"][cav]
        assert np.array_equal(s["lidar_pose"], pose)
        k = len(s["object_ids"])
        assert s["object_bbx_mask"].sum() == k and not s["object_bbx_center"][k:].any()
        local = s["object_bbx_center"][:k].astype(np.float64)
        ego = f["object_bbx_center_valid"][s["object_ids"]]
        assert np.abs(local[:, :3] @ pose[:3, :3].T + pose[:3, 3] - ego[:, :3]).max() < 1e-4
        assert np.abs(_wrap(local[:, 6] + math.atan2(pose[1, 0], pose[0, 0]) - ego[:, 6])).max() < 1e-5
        every = f["object_bbx_center_valid"]
        allb = (np.linalg.inv(pose) @ np.c_[every[:, :3], np.ones(len(every))].T).T
        inside = np.nonzero((allb[:, 0] > rng[0]) & (allb[:, 0] < rng[3]) & (allb[:, 1] > rng[1]) & (allb[:, 1] < rng[4]))[0]
        assert np.array_equal(inside, s["object_ids"])
        lab = s["label_dict"]
        assert lab["pos_equal_one"].shape == (*ds.anchors.shape[:2], 2) and lab["targets"].shape == (*ds.anchors.shape[:2], 14)
        n_pos += int(lab["pos_equal_one"].sum())
    assert n_pos > 0


def test_camera_agent_choice_is_seeded_and_batches_stack():
    from hmvit_amd import trainer as T
    _, a, _ = _camera_dataset(seed=7, n=12)
    _, b, _ = _camera_dataset(seed=7, n=12)
    _, c, _ = _camera_dataset(seed=8, n=12)
    ca = [a.pick_cav(i) for i in range(12)]
    assert ca == [b.pick_cav(i) for i in range(12)] and len(set(ca)) > 1
    assert ca != [c.pick_cav(i) for i in range(12)]
    sa, sb = a[4], b[4]
    assert sa["cav"] == sb["cav"] and torch.equal(sa["camera"], sb["camera"])
    assert np.array_equal(sa["label_dict"]["targets"], sb["label_dict"]["targets"])
    batch = T.to_late_camera_batch(T.Batched(a, 3)[1], None, "cpu")
    assert tuple(batch["camera"].shape) == (3, 4, 32, 32, 3) and tuple(batch["extrinsic"].shape) == (3, 4, 4, 4)
    assert torch.equal(batch["camera"][1], a[4]["camera"])
    assert tuple(batch["label_dict"]["pos_equal_one"].shape) == (3, *a.anchors.shape[:2], 2)


def test_fax_config_helper_matches_the_yaml_and_the_anchor_grid():
    import hmvit_amd
    from hmvit_amd import replay as R
    from hmvit_amd import synthetic as S
    from hmvit_amd.postprocess import VoxelPostprocessor
    # fax_late_fusion.yaml's model block: 512-pixel images, BEV 256, its windows
    c = S.fax_camera_config(512, 512, 512, meters=100.0)
    fax = c["fax"]
    assert fax["bev_embedding"]["bev_height"] == fax["bev_embedding"]["bev_width"] == 256
    assert fax["cross_view_swap"]["q_win_size"] == [[16, 16], [16, 16], [32, 32]]
    assert fax["cross_view_swap"]["feat_win_size"] == [[8, 8], [8, 8], [16, 16]]
    assert fax["self_attn"]["window_size"] == 32 and fax["middle"] == [2, 2, 2] and fax["dim"] == [128, 128, 128]
    assert c["encoder"]["id_pick"] == [1, 2, 3] and c["decoder"]["num_ch_dec"] == [256, 256] and c["anchor_number"] == 2
    for nx, image in ((128, 64), (256, 64), (512, 512), (192, 96)):
        cfg = R.lidar_model_config(nx, nx)
        anchors = VoxelPostprocessor(R.postprocess_params(cfg)).generate_anchor_box()
        c = S.fax_camera_config(nx, nx, image)
        bev = c["fax"]["bev_embedding"]["bev_height"]
        assert (bev // 2, bev // 2) == anchors.shape[:2], nx             # head grid = decoder output = bev / 2 = anchor grid
        net = hmvit_amd.FaxCameraEncoder(c)                                # windows consistent with the ResNet's feature maps
        for i, cv in enumerate(net.fax.cross_views):
            f = net.encoder.output_shapes[i][-1]
            q = bev >> (i + 1)
            assert (q // cv.q_win_size[0]) == (f // cv.feat_win_size[0]), (nx, image, i)
    for nx, ny, image in ((256, 128, 64), (100, 100, 64), (136, 136, 64), (128, 128, 48)):
        with pytest.raises(ValueError):
            S.fax_camera_config(nx, ny, image)


class _Stage2:
    stage, grid, agents, small, precision, seed, frames, train_lidar_backbone = "hetero", [128, 128], 3, True, "f32", 0, 2, False
    val_frames, camera_ratio, ego_mode, camera_image, train_camera_backbone = 0, 0.5, "mixed", 64, False
    camera_encoder, camera_backbone_dir = "fax", None


def test_stage1_camera_keys_load_strictly_into_the_stage2_camera_slot(tmp_path):
    from hmvit_amd import FaxCameraEncoder, FaxFusedTransformer
    from hmvit_amd import trainer as T

    class Stage1:
        stage, grid, agents, seed, frames, batch, val_frames, camera_image = "camera_backbone", [128, 128], 3, 0, 4, None, 0, 64
    cfg, model, pre, post, ds, val = T.build(Stage1)
    assert FaxFusedTransformer is FaxCameraEncoder and type(model) is FaxCameraEncoder and not model.return_features
    assert ds.batch == 3 and len(ds) == 2 and val is None and pre is None      # fax_late_fusion.yaml's batch_size
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.125)
    path = T.save_checkpoint(model, str(tmp_path), 0)
    saved = torch.load(path, map_location="cpu")

    class Stage2(_Stage2):
        camera_backbone_dir = str(tmp_path)
    _, hetero, _, _, _, _ = T.build(Stage2)
    slot = hetero.camera_encoder
    assert type(slot) is FaxCameraEncoder and slot.return_features
    slot.load_state_dict(saved, strict=True)                                 # same keys, heads included
    assert list(slot.state_dict()) == list(saved)
    _, fresh, _, _, _, _ = T.build(Stage2)
    assert all(torch.equal(fresh.camera_encoder.state_dict()[k], saved[k]) for k in saved)     # loaded by --camera_backbone_dir
    assert fresh._fix_camera_backbone

    class Missing(_Stage2):
        camera_backbone_dir = str(tmp_path / "nothing-here")
    with pytest.raises(FileNotFoundError):
        T.build(Missing)


def test_argument_checks_run_before_any_device_work(tmp_path, monkeypatch):
    from hmvit_amd import replay as R
    from hmvit_amd import trainer as T
    touched = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: touched.append(1) or False)
    with pytest.raises(ValueError, match="camera_encoder fax"):
        T.main(["--camera_ratio", "0.5", "--camera_backbone_dir", str(tmp_path)])
    with pytest.raises(ValueError, match="square"):
        T.main(["--stage", "camera_backbone", "--grid", "256", "128"])
    with pytest.raises(ValueError, match="square"):
        T.main(["--camera_ratio", "0.5", "--camera_encoder", "fax", "--grid", "256", "128"])
    with pytest.raises(ValueError):
        R.main(["--late", "--camera_ratio", "0.5", "--grid", "512", "192"])
    assert not touched
    with pytest.raises(SystemExit):                                        # a servable grid gets as far as the device check
        T.main(["--stage", "camera_backbone", "--grid", "128", "128"])
    assert touched

    class NoFax(_Stage2):
        camera_encoder, camera_backbone_dir = "cvt", str(tmp_path)
    with pytest.raises(ValueError, match="camera_encoder fax"):
        T.build(NoFax)


def test_replay_frames_without_camera_agents_are_unchanged():
    """Frames of ``SyntheticReplayDataset`` with camera_ratio 0 against the fixture written by the dataset before it gained the
    modality roll (tests/golden/replay_frames_lidar.npz); ego 'lidar' and 'mixed' give the same frames, without camera tensors."""
    import hmvit_amd  # noqa: F401
    from hmvit_amd import replay as R
    g = np.load(os.path.join(GOLDEN, "replay_frames_lidar.npz"))
    cfg = R.lidar_model_config(32, 32, max_cav=3, small=True)
    for ego in ("lidar", "mixed"):
        ds = R.SyntheticReplayDataset(cfg, 2, n_agents=2, n_obj=4, seed=11, camera_ratio=0.0, ego_mode=ego)
        for i in range(2):
            f = ds[i]
            assert set(f) == {"clouds", "pairwise_t_matrix", "mode", "record_len", "object_bbx_corners", "object_bbx_center_valid",
                              "lidar_poses"}
            for a, c in enumerate(f["clouds"]):
                ref = g[f"f{i}_cloud{a}"]
                assert c.dtype == ref.dtype and c.shape == ref.shape
                assert np.allclose(c, ref, rtol=1e-6, atol=1e-5)
            for k in ("pairwise_t_matrix", "mode", "record_len"):
                assert f[k].dtype == torch.from_numpy(g[f"f{i}_{k}"]).dtype and np.allclose(f[k].numpy(), g[f"f{i}_{k}"], rtol=1e-6, atol=1e-6), k
            for k in ("object_bbx_corners", "object_bbx_center_valid", "lidar_poses"):
                assert np.allclose(np.asarray(f[k]), g[f"f{i}_{k}"], rtol=1e-6, atol=1e-6), k
