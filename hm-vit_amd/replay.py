"""Inference replay on procedurally generated scenes: the per-frame loop of the reference's inference driver
(``opencood/tools/inference_camera.py:145-195``: batch -> model -> ``post_process`` -> ``caluclate_tp_fp`` at IoU 0.3 / 0.5 /
0.7 -> ``calculate_ap``) over a synthetic stand-in for the OPV2V dataset, all of it on the HIP pipeline (pillariser ->
PointPillar -> HeteroFusion -> HeteroDecoder -> heads -> box decode / rotated NMS -> AP arithmetic).

There is no OPV2V data and no trained checkpoint in this environment, so a scene is: vehicles of the anchor size
scattered over the ego's range, every agent (rigid poses T_i, ``pairwise[i, j] = inv(T_j) T_i`` as
``mixed/intermediate_fusion_dataset.py:163-202`` builds them) seeing points on the vehicle surfaces plus ground clutter in
its own frame.  The config dicts carry the keys of the shipped yaml (``opencood/hypes_yaml/opcamera/mixed/hm_vit.yaml``).
With random weights the AP is that of an untrained detector; what the harness provides is the loop, its timing and a place
to load a reference checkpoint (``--checkpoint``: a ``state_dict`` file, loaded ``strict=False`` as ``train_utils.py:66-70``).

    python -m hmvit_amd.replay --scenes 8 --precision f16        (from the repository root)
    python -m hmvit_amd.replay --late --small --checkpoint runs/stage1/net_epoch2.pth     (a stage-1 detector, late fusion)
    python -m hmvit_amd.replay --late --camera_ratio 0.5 --checkpoint runs/stage1/net_epoch2.pth \
        --camera_checkpoint runs/stage1_camera/net_epoch2.pth                             (mixed late fusion; --nofusion: the ego alone)
"""
from __future__ import annotations

import argparse
import json
import math
import time

import numpy as np
import torch

from . import synthetic as S
from .postprocess import boxes_to_corners_3d


def lidar_model_config(nx: int = 512, ny: int = 512, max_cav: int = 5, window: int = 8, small: bool = False) -> dict:
    """LiDAR-only HM-ViT model config with the shipped yaml's structure: 0.4 m pillars on an (nx, ny) grid, PointPillar with
    layer_nums [3, 5, 8] (``small``: [1, 2, 2]), shrink header to 256 channels at 1/4 resolution, fusion with C = 256."""
    lidar = {"voxel_size": [0.4, 0.4, 4], "lidar_range": [-nx * 0.2, -ny * 0.2, -3, nx * 0.2, ny * 0.2, 1],
             "anchor_number": 2, "cls_head_dim": 256,
             "pillar_vfe": {"use_norm": True, "with_distance": False, "use_absolute_xyz": True, "num_filters": [64]},
             "point_pillar_scatter": {"num_features": 64, "grid_size": [nx, ny, 1]},
             "base_bev_backbone": {"layer_nums": [1, 2, 2] if small else [3, 5, 8], "layer_strides": [2, 2, 2],
                                   "num_filters": [64, 128, 256], "upsample_strides": [1, 2, 4],
                                   "num_upsample_filter": [128, 128, 128]},
             "shrink_header": {"kernal_size": [3], "stride": [2], "padding": [1], "dim": [256], "input_dim": 384}}
    st = {"downsample_rate": 4, "voxel_size": [0.4, 0.4, 4], "use_roi_mask": True}
    return {"max_cav": max_cav, "anchor_number": 2, "compression": 0, "spatial_transform": st, "camera": {}, "lidar": lidar,
            "hetero_fusion": S.make_config(256, window, max_cav, voxel=0.4, downsample=4),
            "hetero_decoder": {"input_dim": 256, "num_layer": 2, "num_ch_dec": [256, 256], "anchor_number": 2}}


def preprocess_params(cfg: dict) -> dict:
    la = cfg["lidar"]
    return {"cav_lidar_range": la["lidar_range"],
            "args": {"voxel_size": la["voxel_size"], "max_points_per_voxel": 32, "max_voxel_train": 32000, "max_voxel_test": 70000}}


def postprocess_params(cfg: dict) -> dict:
    la = cfg["lidar"]
    nx, ny = la["point_pillar_scatter"]["grid_size"][:2]
    return {"order": "hwl", "nms_thresh": 0.15, "max_num": 100,
            "target_args": {"score_threshold": 0.27, "pos_threshold": 0.6, "neg_threshold": 0.45},
            "anchor_args": {"cav_lidar_range": la["lidar_range"], "W": nx // 2, "H": ny // 2, "vw": 0.4, "vh": 0.4, "vd": 4,
                            "l": 3.9, "w": 1.6, "h": 1.56, "r": [0, 90], "num": 2, "feature_stride": 2}}


class SyntheticReplayDataset:
    """``len(ds)`` frames; ``ds[i]`` -> {'clouds': [(n_i, 4) float32 per agent], 'pairwise_t_matrix' (1, L, L, 4, 4),
    'mode' (1, L), 'record_len' (1,), 'object_bbx_corners' (n_obj, 8, 3), 'lidar_poses' (L, 4, 4) float64 agent -> ego} - what the
    driver needs from ``batch['ego']``.

    ``camera_ratio`` / ``ego_mode``: the modality roll of ``basedataset.py:193-200`` - every non-ego agent is a camera agent
    with probability ``camera_to_lidar_ratio``, the ego is ``lidar`` / ``camera`` or rolled like the others (``mixed``).  A frame
    with camera agents carries ``camera`` / ``intrinsic`` / ``extrinsic`` / ``cav2cam_extrinsic`` for ALL its agents next to
    the point clouds, as ``collate_batch`` hands them over (``mixed/intermediate_fusion_dataset.py:398-415``); ``mode`` says
    which sensor of an agent the model reads.  Without camera agents (ratio 0, ego not ``camera``) a frame is LiDAR-only."""

    def __init__(self, cfg: dict, n_frames: int, n_agents: int | None = None, n_obj: int = 12, seed: int = 7,
                 camera_ratio: float = 0.0, ego_mode: str = "mixed", camera_image: int = 64):
        self.cfg, self.n_frames, self.n_obj = cfg, n_frames, n_obj
        self.n_agents = n_agents or cfg["max_cav"]
        self.seed = seed
        self.camera_ratio, self.ego_mode, self.camera_image = camera_ratio, ego_mode, camera_image

    def has_cameras(self) -> bool:
        return self.camera_ratio > 0 or self.ego_mode == "camera"

    def roll_modes(self, idx):
        """Per agent 0 (camera) / 1 (LiDAR) of frame ``idx``, seeded by the frame."""
        rs = np.random.RandomState(self.seed + 77 + 1000 * idx)
        m = [0 if rs.uniform() < self.camera_ratio else 1 for _ in range(self.n_agents)]
        if self.ego_mode == "lidar":
            m[0] = 1
        elif self.ego_mode == "camera":
            m[0] = 0
        return m

    def __len__(self):
        return self.n_frames

    def __getitem__(self, idx):
        rs = np.random.RandomState(self.seed + 1000 * idx)
        rng = self.cfg["lidar"]["lidar_range"]
        L = self.n_agents
        span = min(rng[3], rng[4])
        poses = [S.rigid(0.15 * i, 0.06 * span * i, -0.04 * span * i) for i in range(L)]        # agent i -> ego frame
        boxes = np.array([[rs.uniform(rng[0] + 3, rng[3] - 3), rs.uniform(rng[1] + 3, rng[4] - 3), -1.0, 1.56, 1.6, 3.9,
                           rs.uniform(-math.pi, math.pi)] for _ in range(self.n_obj)], np.float32)
        clouds = []
        for i in range(L):
            pts = []
            for b in boxes:
                dims = np.array([b[5], b[4], b[3]])
                u = rs.uniform(-0.5, 0.5, (150, 3)) * dims
                face = rs.randint(0, 3, 150)
                u[np.arange(150), face] = np.sign(u[np.arange(150), face]) * 0.5 * dims[face]
                c, s = math.cos(b[6]), math.sin(b[6])
                pts.append(np.stack([u[:, 0] * c - u[:, 1] * s + b[0], u[:, 0] * s + u[:, 1] * c + b[1], u[:, 2] + b[2]], 1))
            n_ground = 40 * int(rng[3] - rng[0])
            ground = np.stack([rs.uniform(rng[0], rng[3], n_ground), rs.uniform(rng[1], rng[4], n_ground),
                               rs.uniform(-2.6, -2.3, n_ground)], 1)
            world = np.concatenate(pts + [ground]).astype(np.float64)
            Tinv = np.linalg.inv(poses[i].numpy())
            local = (Tinv[:3, :3] @ world.T).T + Tinv[:3, 3]
            clouds.append(np.concatenate([local, rs.uniform(0, 1, (len(local), 1))], 1).astype(np.float32))
        frame = {"clouds": clouds, "pairwise_t_matrix": S.pairwise_from_poses(poses, self.cfg["max_cav"])[None],
                 "mode": torch.ones(1, self.cfg["max_cav"], dtype=torch.float64), "record_len": torch.tensor([L]),
                 "object_bbx_corners": boxes_to_corners_3d(boxes), "object_bbx_center_valid": boxes,
                 "lidar_poses": torch.stack(poses).numpy()}
        if self.has_cameras():
            mode = torch.zeros(1, self.cfg["max_cav"], dtype=torch.float64)       # padding slots: 0 (base_camera_lidar_dataset.py:178)
            mode[0, :L] = torch.tensor(self.roll_modes(idx), dtype=torch.float64)
            frame["mode"] = mode
            frame.update(S.synthetic_cameras(L, self.camera_image, seed=self.seed + 31 + 1000 * idx))
        return frame


def late_inputs(frame: dict, pre, device, nofusion: bool = False) -> dict:
    """The detector inputs of one frame for late fusion: the agents that run (all, or only the ego (agent 0) for ``nofusion``) and
    per modality (``mode`` 1 LiDAR, 0 camera) their agent ids with one batch of their sensor data: the pillars of the LiDAR
    agents' clouds, each in its own frame, and the camera agents' images / intrinsics / extrinsics."""
    L = len(frame["clouds"])
    modes = [int(v) for v in frame["mode"][0, :L].tolist()]
    agents = [0] if nofusion else list(range(L))
    lid = [a for a in agents if modes[a] == 1]
    cam = [a for a in agents if modes[a] == 0]
    inputs = {"agents": agents, "lidar": None, "camera": None}
    if lid:
        inputs["lidar"] = (lid, {"processed_lidar": pre.collate_batch([pre.preprocess(frame["clouds"][a]) for a in lid]),
                                 "n_agents": len(lid)})
    if cam:
        idx = torch.tensor(cam)
        inputs["camera"] = (cam, {k: frame[k][idx].to(device) for k in ("camera", "intrinsic", "extrinsic")})
    return inputs


def late_heads(inputs: dict, lidar_model, camera_model) -> dict:
    """``inference_mixed_late_fusion`` / ``inference_mixed_no_fusion`` (``tools/infrence_utils.py:40-108``) on the inputs of
    ``late_inputs``: the camera agents through ``camera_model`` (the FAX detector) in ONE call, the LiDAR agents through
    ``lidar_model`` (PointPillar) in ONE call; a detector without agents is not called.  The heads are split back per agent ->
    {agent: {'psm' (1, A, H, W), 'rm' (1, 7 A, H, W)}} in agent order."""
    heads = {}
    for key, model in (("lidar", lidar_model), ("camera", camera_model)):
        if inputs[key] is None:
            continue
        ids, batch = inputs[key]
        if model is None:
            raise ValueError(f"this frame has {key} agents but no {key} detector was given")
        out = model(batch)
        heads.update({a: {"psm": out["psm"][j:j + 1], "rm": out["rm"][j:j + 1]} for j, a in enumerate(ids)})
    return {a: heads[a] for a in inputs["agents"]}


def inference(model, dataset, pre, post, calibrate_top: int | None = 200, log=None, late: bool = False, camera_model=None,
              nofusion: bool = False, outputs: list | None = None) -> dict:
    """The driver loop.  ``calibrate_top``: with an untrained head every anchor fires, so the score threshold of each frame
    is set to keep that many anchors (None: the config's threshold, for a trained checkpoint).  ``late``: ``model`` is the
    standalone ``PointPillar`` detector; every agent's cloud goes through it in its own frame (one batch of L samples) and
    ``post_process`` projects each agent's boxes with its agent -> ego ``transformation_matrix`` before the joint NMS
    (``inference_camera.py --fusion_method late``, ``late_fusion_dataset.py`` ``post_process``).  Camera agents of the frame
    (``mode`` 0) go through ``camera_model``, the FAX camera detector (``--mixed_fusion``), see ``late_heads``.  ``nofusion``: the
    ego's detections alone, with the identity transform.  ``outputs``: a list that receives (boxes, scores) of every frame."""
    from .postprocess import calculate_ap, caluclate_tp_fp
    dev = next(model.parameters()).device
    anchors = post.generate_anchor_box()
    thr = (0.3, 0.5, 0.7)
    stat = {t: {"tp": [], "fp": [], "gt": 0} for t in thr}
    n_det, n_cam, t_model, t_post = 0, 0, 0.0, 0.0
    late = late or nofusion
    for i in range(len(dataset)):
        frame = dataset[i]
        if late:
            inputs = late_inputs(frame, pre, dev, nofusion=nofusion)
        else:
            lidar = pre.collate_batch([pre.preprocess(c) for c in frame["clouds"]])
            batch = {"mode": frame["mode"].to(dev), "record_len": frame["record_len"].to(dev),
                     "pairwise_t_matrix": frame["pairwise_t_matrix"].to(dev), "processed_lidar": lidar}
        n_cam += int((frame["mode"][0, :len(frame["clouds"])] == 0).sum())
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if late:
            heads = late_heads(inputs, model, camera_model)
            psm_all = torch.cat([h["psm"].reshape(-1) for h in heads.values()])
        else:
            out = model(batch)
            psm_all = out["psm"]
        torch.cuda.synchronize(dev)
        t1 = time.perf_counter()
        for h in (heads.values() if late else [out]):
            if h["psm"].shape[2:] != anchors.shape[:2]:
                raise RuntimeError(f"anchor grid {anchors.shape[:2]} != head grid {tuple(h['psm'].shape[2:])}")
        if calibrate_top is not None:
            k = max(1, psm_all.numel() - calibrate_top)
            kth = float(torch.sigmoid(psm_all.float()).flatten().kthvalue(k).values)
            post.params["target_args"]["score_threshold"] = float(np.nextafter(np.float32(min(kth, 1.0)), np.float32(0)))
        if late:
            poses = torch.from_numpy(frame["lidar_poses"]).float()
            # inference_mixed_no_fusion: the ego's boxes stay in its own frame (the identity)
            data = {a: {"anchor_box": torch.from_numpy(anchors), "transformation_matrix": torch.eye(4) if nofusion else poses[a]}
                    for a in heads}
        else:
            data = {"ego": {"anchor_box": torch.from_numpy(anchors), "transformation_matrix": torch.eye(4)}}
            heads = {"ego": {"psm": out["psm"], "rm": out["rm"]}}
        boxes, scores = post.post_process(data, heads)
        torch.cuda.synchronize(dev)
        t2 = time.perf_counter()
        if outputs is not None:
            outputs.append((boxes, scores))
        gt = torch.from_numpy(frame["object_bbx_corners"]).to(dev)
        for t in thr:
            caluclate_tp_fp(boxes, scores, gt, stat, t)
        n_det += 0 if boxes is None else len(boxes)
        if i > 0:                      # the first frame carries the weight preparation
            t_model += t1 - t0
            t_post += t2 - t1
        if log:
            log(f"frame {i}: {0 if boxes is None else len(boxes)} boxes, model {1e3 * (t1 - t0):.2f} ms, post {1e3 * (t2 - t1):.2f} ms")
    n = max(1, len(dataset) - 1)
    res = {"frames": len(dataset), "detections": n_det, "model_ms_per_frame": 1e3 * t_model / n,
           "postprocess_ms_per_frame": 1e3 * t_post / n, "camera_agents": n_cam}
    for t in thr:
        res[f"AP@{t}"] = round(100 * calculate_ap(stat, t)[0], 3) if stat[t]["tp"] else 0.0
    return res


def _damp_untrained_heads(model):
    """Untrained weights: keep the regression deltas small so that the decoded boxes stay anchor-like and survive the
    post-processor's size filters (a random head otherwise decodes to boxes hundreds of metres long)."""
    with torch.no_grad():
        model.reg_head.weight.mul_(0.02)
        model.reg_head.bias.zero_()
        model.cls_head.weight.mul_(0.05)       # and the logits out of the sigmoid's saturated range (distinct scores)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--grid", type=int, nargs=2, default=None, metavar=("NX", "NY"),
                    help="pillar grid (0.4 m cells); default 512 x 192, which keeps the map inside the evaluation range |y| <= 40 m "
                         "(boxes outside it are dropped by the post-processor as in the reference), and 256 x 256 when there are "
                         "camera agents (the FAX camera detector needs a square grid)")
    ap.add_argument("--precision", default="f16", choices=["f16", "f32"])
    ap.add_argument("--small", action="store_true", help="PointPillar layer_nums [1, 2, 2] (as the trainer's --small)")
    ap.add_argument("--checkpoint", default=None, help="state_dict file of the reference model (loaded strict=False); with --late / "
                                                        "--nofusion the LiDAR detector's")
    ap.add_argument("--late", action="store_true",
                    help="late fusion: the standalone PointPillar detector per agent (a --stage lidar_backbone checkpoint of "
                         "hmvit_amd.trainer), boxes projected to the ego and merged by the NMS")
    ap.add_argument("--nofusion", action="store_true",
                    help="no fusion: only the ego's detector runs, the ego's boxes alone (inference_mixed_no_fusion)")
    ap.add_argument("--camera_ratio", type=float, default=0.0,
                    help="camera_to_lidar_ratio of the modality roll (--late / --nofusion): camera agents run the FAX camera detector")
    ap.add_argument("--ego_mode", default="mixed", choices=["mixed", "lidar", "camera"])
    ap.add_argument("--camera_image", type=int, default=64, help="camera image size of the synthetic frames")
    ap.add_argument("--camera_checkpoint", default=None,
                    help="net_epoch%%d.pth of hmvit_amd.trainer --stage camera_backbone: the camera detector's weights")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--verbose", action="store_true")
    args = ap.parse_args(argv)
    from . import BevformerPointPillarHetero, FaxCameraEncoder, PointPillar, SpVoxelPreprocessor, VoxelPostprocessor
    late = args.late or args.nofusion
    cameras = args.camera_ratio > 0 or args.ego_mode == "camera"
    if cameras and not late:
        raise ValueError("camera agents (--camera_ratio > 0 or --ego_mode camera) need --late or --nofusion")
    if args.grid is None:
        args.grid = [256, 256] if cameras else [512, 192]
    ccfg = S.fax_camera_config(args.grid[0], args.grid[1], args.camera_image) if cameras else None     # ValueError before GPU work
    if not torch.cuda.is_available():
        raise SystemExit("hm-vit_amd has no CPU path: this needs an MI355X")
    cfg = lidar_model_config(args.grid[0], args.grid[1], max_cav=args.agents, small=args.small)
    torch.manual_seed(args.seed)
    if late:
        model = PointPillar(cfg["lidar"], precision=args.precision)
    else:
        model = BevformerPointPillarHetero(cfg, precision=args.precision)
    if args.checkpoint:
        missing, unexpected = model.load_state_dict(torch.load(args.checkpoint, map_location="cpu"), strict=False)
        print(f"checkpoint: {len(missing)} missing / {len(unexpected)} unexpected keys")
    else:
        _damp_untrained_heads(model)
    model = model.cuda().eval()
    camera_model = None
    if cameras:
        camera_model = FaxCameraEncoder(ccfg, precision=args.precision)
        if args.camera_checkpoint:
            missing, unexpected = camera_model.load_state_dict(torch.load(args.camera_checkpoint, map_location="cpu"), strict=False)
            print(f"camera checkpoint: {len(missing)} missing / {len(unexpected)} unexpected keys")
        else:
            _damp_untrained_heads(camera_model)
        camera_model = camera_model.cuda().eval()
    pre = SpVoxelPreprocessor(preprocess_params(cfg), train=False)
    post = VoxelPostprocessor(postprocess_params(cfg), train=False)
    ds = SyntheticReplayDataset(cfg, args.scenes, n_agents=args.agents, seed=args.seed + 7, camera_ratio=args.camera_ratio,
                                ego_mode=args.ego_mode, camera_image=args.camera_image)
    trained = args.checkpoint and (args.camera_checkpoint or not cameras)
    res = inference(model, ds, pre, post, calibrate_top=None if trained else 200, log=print if args.verbose else None,
                    late=late, camera_model=camera_model, nofusion=args.nofusion)
    res.update(precision=args.precision, agents=args.agents, grid=args.grid,
               fusion="nofusion" if args.nofusion else "late" if args.late else "intermediate", camera_ratio=args.camera_ratio,
               ego_mode=args.ego_mode)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
