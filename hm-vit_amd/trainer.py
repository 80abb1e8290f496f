"""Minimal train harness: the loop of the reference's ``opencood/tools/train_camera.py:43-230`` over the
synthetic replay scenes, one process per GPU with the gradient all-reduce on RCCL.

What it mirrors, piece by piece (citations into /root/reference/opencood):
  * process group      ``tools/multi_gpu_utils.py:16-37``   RANK / WORLD_SIZE / LOCAL_RANK from the launcher, backend "nccl"
                                                             (= RCCL over xGMI on ROCm), one device per process;
  * model wrapping     ``tools/train_camera.py:118-131``    ``fix_lidar_backbone()`` then
                                                             ``DistributedDataParallel(model, device_ids=[gpu], find_unused_parameters=True)``
                                                             (the parameters of agent types absent from a batch, ``aggregate_fc`` and the
                                                             unused ``cls_head`` / ``reg_head`` get no gradient);
  * loss / optimiser   ``tools/train_utils.py:146-230``     ``PointPillarLoss`` (hm-vit_amd/train.py), AdamW lr 2e-4 eps 1e-10 wd 1e-2;
  * lr schedule        ``tools/train_utils.py:247-264``     timm's ``CosineLRScheduler`` (third party, absent, version unpinned:
                                                             ``cosine_lr.py`` restated from its published formula, parity unpinned),
                                                             stepped per iteration with ``step_update(epoch * num_steps + i)``;
  * per-batch step     ``tools/train_camera.py:163-199``    ``model.train(); zero_grad(); out = model(batch['ego']);
                                                             loss = criterion(out, label_dict); loss.backward(); optimizer.step()``;
  * checkpoints        ``tools/train_camera.py:221-225``, ``tools/train_utils.py:40-75``: ``net_epoch%d.pth`` = ``state_dict()`` of the
                                                             un-wrapped model every ``save_freq`` epochs; resuming loads the highest epoch
                                                             found in the folder with ``strict=False``;
  * labels             ``data_utils/post_processor/voxel_postprocessor.py:74-229`` (hm-vit_amd/postprocess.py ``generate_label``).

What trains on which code: the fusion (the hot path) runs its HIP forward AND backward kernels (hm-vit_amd/train.py); the LiDAR
encoder runs frozen on its HIP inference kernels (``fix_lidar_backbone``, the reference's own option, the default here) or trains
on libhmvit too (``--train_lidar_backbone``, hm-vit_amd/encoder_train.py);
the detection tail (``HeteroDecoder``: four 3x3 convolutions + BatchNorm in batch-statistics mode + ReLU + two 1x1 heads) runs
HIP forward and backward kernels as well (hm-vit_amd/tail_train.py).

The two stages of the reference's recipe: stage 1 (``--stage lidar_backbone``, ``opcl/point_pillar_late_fusion.yaml``) trains the
standalone PointPillar detector on single-agent samples (``LateFusionTrainDataset``: one random agent per frame, in its own frame,
``late_fusion_dataset.py:33-49``) with ``FusedPointPillarLoss``; ``--stage camera_backbone`` (``opcl/fax_late_fusion.yaml``) does the
same for the FAX camera detector on single camera-agent samples; stage 2 (the default ``--stage hetero``) loads those checkpoints
into ``model.lidar_encoder`` (``--lidar_backbone_dir``, ``train_camera.py:109-114``) and, with ``--camera_encoder fax``, into
``model.camera_encoder`` (``--camera_backbone_dir``) and freezes them.

    python -m hmvit_amd.trainer --epochs 2 --frames 8                      (one GPU)
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m hmvit_amd.trainer --epochs 2
    python -m hmvit_amd.trainer --stage lidar_backbone --model_dir runs/stage1          (stage 1)
    python -m hmvit_amd.trainer --lidar_backbone_dir runs/stage1 --model_dir runs/stage2 (stage 2)
    python -m hmvit_amd.trainer --stage camera_backbone --grid 256 256 --model_dir runs/stage1_camera   (camera stage 1)
"""
from __future__ import annotations

import argparse
import glob
import json
import math
import os
import re
import time

import numpy as np
import torch

from . import replay as R
from .train import FusedPointPillarLoss, PointPillarLoss, make_optimizer


# ---------------------------------------------------------------------------------------------------------------------
# schedule, optimiser, loss, checkpoints: pure host logic (tests/test_train_cpu.py)
# ---------------------------------------------------------------------------------------------------------------------
class CosineLRScheduler:
    """timm ``CosineLRScheduler(optimizer, t_initial, lr_min, warmup_lr_init, warmup_t, cycle_limit=1, t_in_epochs=False)`` as
    ``setup_lr_schedular`` constructs it: for update t < warmup_t the rate moves linearly from ``warmup_lr_init`` to the base
    rate, afterwards ``lr_min + (base - lr_min) (1 + cos(pi t / t_initial)) / 2`` (t NOT shifted by the warm-up: timm's
    ``warmup_prefix=False``), and ``lr_min`` once t >= t_initial.  The shipped yaml warms DOWN (warmup_lr 2e-3 > lr 2e-4)."""

    def __init__(self, optimizer, t_initial: int, lr_min: float = 0.0, warmup_lr_init: float = 0.0, warmup_t: int = 0):
        self.optimizer, self.t_initial, self.lr_min = optimizer, max(1, int(t_initial)), lr_min
        self.warmup_lr_init, self.warmup_t = warmup_lr_init, int(warmup_t)
        self.base = [g["lr"] for g in optimizer.param_groups]
        if self.warmup_t:
            for g in optimizer.param_groups:
                g["lr"] = warmup_lr_init

    def lr_at(self, t: int):
        if t < self.warmup_t:
            return [self.warmup_lr_init + t * (b - self.warmup_lr_init) / self.warmup_t for b in self.base]
        if t >= self.t_initial:
            return [self.lr_min for _ in self.base]
        return [self.lr_min + 0.5 * (b - self.lr_min) * (1 + math.cos(math.pi * t / self.t_initial)) for b in self.base]

    def step_update(self, num_updates: int):
        for g, lr in zip(self.optimizer.param_groups, self.lr_at(num_updates)):
            g["lr"] = lr

    def step(self, epoch: int):        # timm steps per epoch only when t_in_epochs; the reference uses step_update
        pass


def default_hypes(epoches: int = 2) -> dict:
    """The train-related blocks of opcl/bevformer_point_pillar_hetero.yaml (:11-20, 156-176)."""
    return {"train_params": {"batch_size": 1, "epoches": epoches, "eval_freq": 1, "save_freq": 1, "max_cav": 5},
            "loss": {"core_method": "point_pillar_loss", "args": {"cls_weight": 1.0, "reg": 2.0}},
            "optimizer": {"core_method": "AdamW", "lr": 2e-4, "args": {"eps": 1e-10, "weight_decay": 1e-2}},
            "lr_scheduler": {"core_method": "cosineannealwarm", "epoches": epoches, "warmup_lr": 2e-3, "warmup_epoches": 10,
                             "lr_min": 5e-6}}


def create_loss(hypes: dict):
    """``point_pillar_loss``: the elementwise torch ``PointPillarLoss``, or with ``hypes['loss']['fused']`` the same loss as one HIP
    kernel pair (``FusedPointPillarLoss``)."""
    if hypes["loss"]["core_method"] != "point_pillar_loss":
        raise NotImplementedError(f"loss {hypes['loss']['core_method']}: only point_pillar_loss is built")
    cls = FusedPointPillarLoss if hypes["loss"].get("fused", False) else PointPillarLoss
    return cls(hypes["loss"]["args"])


def setup_optimizer(hypes: dict, model):
    if hypes["optimizer"]["core_method"] != "AdamW":
        raise NotImplementedError("optimizer: the shipped yaml's AdamW")
    return make_optimizer(model.parameters(), hypes["optimizer"])


def setup_lr_schedular(hypes: dict, optimizer, n_iter_per_epoch: int):
    c = hypes["lr_scheduler"]
    if c["core_method"] == "cosineannealwarm":
        return CosineLRScheduler(optimizer, t_initial=c["epoches"] * n_iter_per_epoch, lr_min=c["lr_min"],
                                 warmup_lr_init=c["warmup_lr"], warmup_t=c["warmup_epoches"] * n_iter_per_epoch)
    raise NotImplementedError(f"lr_scheduler {c['core_method']}: only cosineannealwarm (the shipped yaml) is built")


def save_checkpoint(model, saved_path: str, epoch: int) -> str:
    """``torch.save(model_without_ddp.state_dict(), 'net_epoch%d.pth' % (epoch + 1))``."""
    os.makedirs(saved_path, exist_ok=True)
    path = os.path.join(saved_path, "net_epoch%d.pth" % (epoch + 1))
    torch.save(getattr(model, "module", model).state_dict(), path)
    return path


def load_saved_model(saved_path: str, model):
    """train_utils.py:40-75: the highest ``net_epoch%d.pth`` in the folder, ``strict=False``; returns (epoch, model)."""
    if not os.path.exists(saved_path):
        raise FileNotFoundError("{} not found".format(saved_path))
    epochs = [int(m.group(1)) for f in glob.glob(os.path.join(saved_path, "*epoch*.pth"))
              if (m := re.search(r"epoch(\d+)\.pth$", f))]
    initial = max(epochs) if epochs else 0
    if initial > 0:
        state = torch.load(os.path.join(saved_path, "net_epoch%d.pth" % initial), map_location="cpu")
        model.load_state_dict(state, strict=False)
    return initial, model


def init_distributed_mode(backend: str = "nccl") -> dict:
    """multi_gpu_utils.py:16-37 for a torchrun launch on one node; rendezvous on 127.0.0.1 unless the launcher says otherwise.
    ``backend="gloo"`` with more ranks than GPUs (ranks then share devices) is the 1-GPU rehearsal of the loop; "nccl" is RCCL."""
    if "RANK" not in os.environ or "WORLD_SIZE" not in os.environ:
        return {"distributed": False, "rank": 0, "world_size": 1, "gpu": 0}
    import torch.distributed as dist
    rank, world, gpu = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", 0))
    gpu %= max(1, torch.cuda.device_count())
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    torch.cuda.set_device(gpu)
    dist.init_process_group(backend=backend, init_method="env://", world_size=world, rank=rank)
    dist.barrier()
    return {"distributed": True, "rank": rank, "world_size": world, "gpu": gpu}


# ---------------------------------------------------------------------------------------------------------------------
# data: the replay scenes with anchor targets
# ---------------------------------------------------------------------------------------------------------------------
class SyntheticTrainDataset(R.SyntheticReplayDataset):
    """``ds[i]`` of the replay dataset plus what ``collate_batch_train`` adds for training
    (``mixed/intermediate_fusion_dataset.py:398-415``): ``object_bbx_center`` / ``object_bbx_mask`` padded to ``max_num`` and the
    ``label_dict`` of ``VoxelPostprocessor.generate_label`` on the ego's anchors."""

    def __init__(self, cfg, n_frames, post, n_agents=None, n_obj=12, seed=7, max_num=100, camera_ratio: float = 0.0,
                 ego_mode: str = "mixed", camera_image: int = 64):
        """``camera_ratio`` / ``ego_mode`` / ``camera_image``: the modality roll and camera tensors of the replay frames
        (``SyntheticReplayDataset``)."""
        super().__init__(cfg, n_frames, n_agents=n_agents, n_obj=n_obj, seed=seed, camera_ratio=camera_ratio, ego_mode=ego_mode,
                         camera_image=camera_image)
        self.post, self.max_num = post, max_num
        self.anchors = post.generate_anchor_box()

    def __getitem__(self, idx):
        frame = super().__getitem__(idx)
        boxes = frame["object_bbx_center_valid"]
        center = np.zeros((self.max_num, 7), np.float32)
        mask = np.zeros(self.max_num, np.float32)
        center[: len(boxes)], mask[: len(boxes)] = boxes, 1
        frame["object_bbx_center"], frame["object_bbx_mask"] = center, mask
        frame["label_dict"] = self.post.collate_batch([self.post.generate_label(gt_box_center=center, anchors=self.anchors,
                                                                                mask=mask)])
        return frame


def cav_frame_boxes(boxes: np.ndarray, pose: np.ndarray) -> np.ndarray:
    """(n, 7) [x, y, z, h, w, l, yaw] boxes of the ego frame -> the frame of the agent whose agent -> ego pose is ``pose`` (4, 4):
    centre by the inverse pose, yaw minus the pose's yaw (wrapped to [-pi, pi))."""
    b = np.asarray(boxes, np.float64).copy()
    inv = np.linalg.inv(np.asarray(pose, np.float64))
    b[:, 0:3] = b[:, 0:3] @ inv[:3, :3].T + inv[:3, 3]
    yaw = b[:, 6] - math.atan2(pose[1, 0], pose[0, 0])
    b[:, 6] = (yaw + math.pi) % (2 * math.pi) - math.pi
    return b.astype(np.float32)


class LateFusionTrainDataset(R.SyntheticReplayDataset):
    """The training side of ``CamLiLateFusionDataset`` (``mixed/late_fusion_dataset.py:33-49``) on the synthetic frames: sample
    ``i`` is ONE agent of frame ``i``, drawn with a seeded generator, in that agent's own frame - its point cloud as it sees it, the
    boxes moved into its frame (``cav_frame_boxes``) and kept when their centre lies inside its range (the reference's
    ``mask_boxes_outside_range_numpy``), padded to ``max_num``, and the ``generate_label`` targets of its anchors.

    ``modality="camera"``: the camera detector's samples (``fax_late_fusion.yaml``: camera_to_lidar_ratio 1, ego camera) - every
    agent of the frame is a camera agent and the sample carries the picked agent's four images, intrinsics and camera -> agent
    extrinsics (``camera`` (4, H, W, 3), ``intrinsic`` (4, 3, 3), ``extrinsic`` (4, 4, 4)) instead of its cloud."""

    def __init__(self, cfg, n_samples, post, n_agents=None, n_obj=12, seed=7, max_num=100, modality: str = "lidar",
                 camera_image: int = 64):
        if modality not in ("lidar", "camera"):
            raise ValueError(f"modality must be 'lidar' or 'camera', got {modality!r}")
        cam = modality == "camera"
        super().__init__(cfg, n_samples, n_agents=n_agents, n_obj=n_obj, seed=seed, camera_ratio=1.0 if cam else 0.0,
                         ego_mode="camera" if cam else "mixed", camera_image=camera_image)
        self.post, self.max_num, self.modality = post, max_num, modality
        self.anchors = post.generate_anchor_box()

    def pick_cav(self, idx) -> int:
        return int(np.random.RandomState(self.seed + 13 + 1000 * idx).randint(self.n_agents))

    def __getitem__(self, idx):
        frame = super().__getitem__(idx)
        cav = self.pick_cav(idx)
        pose = frame["lidar_poses"][cav]
        boxes = cav_frame_boxes(frame["object_bbx_center_valid"], pose)
        rng = self.cfg["lidar"]["lidar_range"]
        keep = np.nonzero((boxes[:, 0] > rng[0]) & (boxes[:, 0] < rng[3]) & (boxes[:, 1] > rng[1]) & (boxes[:, 1] < rng[4]))[0]
        keep = keep[: self.max_num]
        center = np.zeros((self.max_num, 7), np.float32)
        mask = np.zeros(self.max_num, np.float32)
        center[: len(keep)], mask[: len(keep)] = boxes[keep], 1
        label = self.post.generate_label(gt_box_center=center, anchors=self.anchors, mask=mask)
        sensor = ({k: frame[k][cav] for k in ("camera", "intrinsic", "extrinsic")} if self.modality == "camera"
                  else {"cloud": frame["clouds"][cav]})
        return {**sensor, "cav": cav, "lidar_pose": pose, "object_ids": keep, "object_bbx_center": center,
                "object_bbx_mask": mask, "label_dict": label}


class Batched:
    """``len(ds) / batch`` batches of consecutive samples (the last one shorter), as a ``DataLoader(batch_size=batch)`` without
    shuffling hands them to ``collate_batch_train``."""

    def __init__(self, ds, batch: int):
        self.ds, self.batch = ds, max(1, int(batch))

    def __len__(self):
        return (len(self.ds) + self.batch - 1) // self.batch

    def __getitem__(self, i):
        return [self.ds[j] for j in range(i * self.batch, min(len(self.ds), (i + 1) * self.batch))]


def to_late_batch(samples: list, pre, device) -> dict:
    """A list of ``LateFusionTrainDataset`` samples -> the standalone detector's batch: every sample's pillars under its own batch
    index (``collate_batch``), ``n_agents`` = the batch size, and the stacked ``label_dict``."""
    from .postprocess import VoxelPostprocessor
    lidar = pre.collate_batch([pre.preprocess(s["cloud"]) for s in samples])
    label = VoxelPostprocessor.collate_batch([s["label_dict"] for s in samples])
    return {"processed_lidar": lidar, "n_agents": len(samples),
            "label_dict": {k: v.to(device=device, dtype=torch.float32) for k, v in label.items()}}


def to_late_camera_batch(samples: list, pre, device) -> dict:
    """A list of camera ``LateFusionTrainDataset`` samples -> the camera detector's batch: ``camera`` (B, 4, H, W, 3), ``intrinsic``
    (B, 4, 3, 3), ``extrinsic`` (B, 4, 4, 4) on the device and the stacked ``label_dict`` (``pre`` is not used: no point clouds)."""
    from .postprocess import VoxelPostprocessor
    label = VoxelPostprocessor.collate_batch([s["label_dict"] for s in samples])
    batch = {k: torch.stack([s[k] for s in samples]).to(device=device, dtype=torch.float32) for k in ("camera", "intrinsic", "extrinsic")}
    batch["label_dict"] = {k: v.to(device=device, dtype=torch.float32) for k, v in label.items()}
    return batch


def to_batch(frame: dict, pre, device) -> dict:
    """One frame -> the ``batch['ego']`` dict the model and the criterion take (pillarisation on the device, csrc/vox.hip)."""
    lidar = pre.collate_batch([pre.preprocess(c) for c in frame["clouds"]])
    label = {k: v.to(device=device, dtype=torch.float32) for k, v in frame["label_dict"].items()}
    batch = {"mode": frame["mode"].to(device), "record_len": frame["record_len"].to(device),
             "pairwise_t_matrix": frame["pairwise_t_matrix"].to(device), "processed_lidar": lidar, "label_dict": label}
    for k in ("camera", "intrinsic", "extrinsic", "cav2cam_extrinsic"):
        if k in frame:
            batch[k] = frame[k].to(device)
    return batch


# ---------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------
def validate(model, val_dataset, pre, criterion, device, batch_fn=to_batch) -> float:
    """The validation pass of ``train_camera.py:201-220``: ``model.eval()`` per batch, ``torch.no_grad()``, mean of the
    criterion over the validation frames (every rank runs the whole split, as the reference's un-sharded ``val_loader``).
    ``eval()`` flips the swapped-in modules to their inference kernels (BatchNorm running statistics, no dropout, the fused
    fusion launch) and ``train()`` at the top of the next step flips them back."""
    losses = []
    with torch.no_grad():
        for i in range(len(val_dataset)):
            model.eval()
            batch = batch_fn(val_dataset[i], pre, device)
            losses.append(float(criterion(model(batch), batch["label_dict"])))
    return sum(losses) / max(1, len(losses))


def train(model, dataset, pre, hypes: dict, saved_path: str | None = None, init_epoch: int = 0, dist_info: dict | None = None,
          log=None, val_dataset=None, batch_fn=to_batch) -> dict:
    """train_camera.py:133-230 (no tensorboard or AMP).  Frames shard over ranks as ``DistributedSampler`` does (rank r takes
    frames r, r + world, ...; the permutation is reseeded per epoch by ``set_epoch``); ``val_dataset``: the validation split,
    run every ``eval_freq`` epochs (:201-220).  ``batch_fn(item, pre, device)``: a dataset item -> the model's batch with its
    ``label_dict`` (``to_batch``; ``to_late_batch`` for the standalone detector of stage 1)."""
    info = dist_info or {"distributed": False, "rank": 0, "world_size": 1, "gpu": 0}
    device = next(model.parameters()).device
    model_without_ddp = model
    if info["distributed"]:
        model = torch.nn.parallel.DistributedDataParallel(model, device_ids=[info["gpu"]], find_unused_parameters=True)
        model_without_ddp = model.module
    criterion = create_loss(hypes)
    optimizer = setup_optimizer(hypes, model_without_ddp)
    world, rank = info["world_size"], info["rank"]
    num_steps = (len(dataset) + world - 1) // world
    scheduler = setup_lr_schedular(hypes, optimizer, num_steps)
    epoches = hypes["train_params"]["epoches"]
    history, val_history, t_step, n_step = [], [], 0.0, 0
    for epoch in range(init_epoch, max(epoches, init_epoch)):
        order = np.random.RandomState(epoch).permutation(len(dataset)) if world > 1 else np.arange(len(dataset))
        mine = [int(order[(rank + k * world) % len(order)]) for k in range(num_steps)]      # padded like DistributedSampler
        losses = []
        for i, idx in enumerate(mine):
            batch = batch_fn(dataset[idx], pre, device)
            torch.cuda.synchronize(device)
            t0 = time.perf_counter()
            model.train()
            model.zero_grad()
            optimizer.zero_grad()
            out = model(batch)
            loss = criterion(out, batch["label_dict"])
            loss.backward()
            optimizer.step()
            scheduler.step_update(epoch * num_steps + i)
            torch.cuda.synchronize(device)
            if epoch > init_epoch or i > 0:               # the first step carries the weight preparation
                t_step += time.perf_counter() - t0
                n_step += 1
            losses.append(float(loss.detach()))
            if log:
                log(f"[epoch {epoch}][{i + 1}/{num_steps}] loss {losses[-1]:.4f} conf {float(criterion.loss_dict['conf_loss']):.4f} "
                    f"loc {float(criterion.loss_dict['reg_loss']):.4f} lr {optimizer.param_groups[0]['lr']:.2e}")
        history.append(sum(losses) / len(losses))
        if val_dataset is not None and epoch % hypes["train_params"]["eval_freq"] == 0:
            val = validate(model, val_dataset, pre, criterion, device, batch_fn)
            val_history.append(val)
            if log:
                log("At epoch %d, the validation loss is %f" % (epoch, val))
        if saved_path and rank == 0 and epoch % hypes["train_params"]["save_freq"] == 0:
            save_checkpoint(model_without_ddp, saved_path, epoch)
    res = {"epoch_loss": history, "val_loss": val_history, "ms_per_step": 1e3 * t_step / max(1, n_step), "steps": n_step,
           "world_size": world}
    if info["distributed"]:
        # after the last step every rank must hold the same parameters (DDP averaged every gradient): largest difference between
        # the ranks' trainable parameters, relative to their largest magnitude - 0 when the all-reduce did its job
        import torch.distributed as dist
        flat = torch.cat([p.detach().float().reshape(-1) for p in model_without_ddp.parameters() if p.requires_grad])
        hi, lo = flat.clone(), flat.clone()
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        res["rank_param_spread"] = float((hi - lo).abs().max() / flat.abs().max().clamp_min(1e-30))
    return res


def build_lidar_backbone(args):
    """Stage 1 (``point_pillar_late_fusion.yaml``): the standalone PointPillar detector and batches of single-agent samples."""
    from . import PointPillar, SpVoxelPreprocessor, VoxelPostprocessor
    cfg = R.lidar_model_config(args.grid[0], args.grid[1], max_cav=args.agents, small=args.small)
    torch.manual_seed(args.seed)
    model = PointPillar(cfg["lidar"])
    pre = SpVoxelPreprocessor(R.preprocess_params(cfg), train=True)
    post = VoxelPostprocessor(R.postprocess_params(cfg), train=True)
    batch = getattr(args, "batch", 8)
    ds = Batched(LateFusionTrainDataset(cfg, args.frames, post, n_agents=args.agents, seed=args.seed + 7), batch)
    val = (Batched(LateFusionTrainDataset(cfg, args.val_frames, post, n_agents=args.agents, seed=args.seed + 100007), batch)
           if args.val_frames > 0 else None)
    return cfg, model, pre, post, ds, val


def camera_detector_config(args) -> dict:
    """``FaxCameraEncoder`` config of ``--grid`` / ``--camera_image`` (``synthetic.fax_camera_config``: raises ``ValueError`` for a
    grid the FAX windows cannot tile)."""
    from . import synthetic as S
    return S.fax_camera_config(args.grid[0], args.grid[1], args.camera_image)


def check_args(args) -> None:
    """The argument checks that need no GPU: run before any device work (``main``) and by ``build``."""
    stage = getattr(args, "stage", "hetero")
    fax = getattr(args, "camera_encoder", "cvt") == "fax"
    if getattr(args, "camera_backbone_dir", None):
        if stage != "hetero" or not fax:
            raise ValueError("--camera_backbone_dir loads a --stage camera_backbone checkpoint into the FAX camera slot: it needs "
                             "--stage hetero with --camera_encoder fax")
        if not (args.camera_ratio > 0 or args.ego_mode == "camera"):
            raise ValueError("--camera_backbone_dir: no camera agents, so no camera slot (pass --camera_ratio > 0 or --ego_mode camera)")
    if stage == "camera_backbone" or (stage == "hetero" and fax):
        camera_detector_config(args)


def build_camera_backbone(args):
    """Stage 1 of the camera half (``fax_late_fusion.yaml``): the standalone FAX camera detector and batches of single camera-agent
    samples.  Returns (cfg, model, pre, post, ds, val) like ``build_lidar_backbone``; ``pre`` is None (no point clouds)."""
    from . import FaxCameraEncoder, VoxelPostprocessor
    cfg = R.lidar_model_config(args.grid[0], args.grid[1], max_cav=args.agents, small=getattr(args, "small", False))
    ccfg = camera_detector_config(args)
    torch.manual_seed(args.seed)
    model = FaxCameraEncoder(ccfg)
    post = VoxelPostprocessor(R.postprocess_params(cfg), train=True)
    batch = getattr(args, "batch", None) or 3
    kw = dict(n_agents=args.agents, modality="camera", camera_image=args.camera_image)
    ds = Batched(LateFusionTrainDataset(cfg, args.frames, post, seed=args.seed + 7, **kw), batch)
    val = (Batched(LateFusionTrainDataset(cfg, args.val_frames, post, seed=args.seed + 100007, **kw), batch)
           if args.val_frames > 0 else None)
    return cfg, model, None, post, ds, val


def build(args):
    from . import BevformerPointPillarHetero, SpVoxelPreprocessor, VoxelPostprocessor
    check_args(args)
    stage = getattr(args, "stage", "hetero")
    if stage == "lidar_backbone":
        return build_lidar_backbone(args)
    if stage == "camera_backbone":
        return build_camera_backbone(args)
    cfg = R.lidar_model_config(args.grid[0], args.grid[1], max_cav=args.agents, small=args.small)
    torch.manual_seed(args.seed)
    camera_encoder = None
    mixed = args.camera_ratio > 0 or args.ego_mode == "camera"
    if mixed:
        # camera agents: the CVT lift (default) or the FAX detector's trunk (--camera_encoder fax) in the model's camera slot,
        # producing the LiDAR branch's (256, ny / 4, nx / 4) BEV map; frozen (train_camera.py's --fix_camera_backbone) unless
        # --train_camera_backbone puts it on the tape (hm-vit_amd/camera_train.py, fax_train.py)
        from . import synthetic as S
        prec = "f32" if args.precision == "f32" else "f16"
        if getattr(args, "camera_encoder", "cvt") == "fax":
            from .fax import FaxCameraEncoder
            camera_encoder = FaxCameraEncoder(camera_detector_config(args), precision=prec)
        else:
            from .camera import CvtCameraEncoder
            camera_encoder = CvtCameraEncoder(S.camera_config(args.camera_image, 18, bev_h=args.grid[1] // 2, bev_w=args.grid[0] // 2),
                                              precision=prec)
    model = BevformerPointPillarHetero(cfg, camera_encoder=camera_encoder, precision=args.precision)
    if getattr(args, "camera_backbone_dir", None):
        # train_camera.py:109-111: the stage-1 camera detector's weights into the camera slot (same module, same keys)
        epoch, _ = load_saved_model(args.camera_backbone_dir, model.camera_encoder)
        if epoch == 0:
            raise FileNotFoundError(f"no net_epoch*.pth in {args.camera_backbone_dir}")
    if mixed and not getattr(args, "train_camera_backbone", False):
        model.fix_camera_backbone()                     # train_camera.py --fix_camera_backbone (the default here: faster steps)
    if getattr(args, "lidar_backbone_dir", None):
        # train_camera.py:109-114: the stage-1 detector's weights into the LiDAR encoder (same module, same keys)
        epoch, _ = load_saved_model(args.lidar_backbone_dir, model.lidar_encoder)
        if epoch == 0:
            raise FileNotFoundError(f"no net_epoch*.pth in {args.lidar_backbone_dir}")
    if not args.train_lidar_backbone:
        model.fix_lidar_backbone()
    pre = SpVoxelPreprocessor(R.preprocess_params(cfg), train=True)
    post = VoxelPostprocessor(R.postprocess_params(cfg), train=True)
    kw = dict(n_agents=args.agents, camera_ratio=args.camera_ratio, ego_mode=args.ego_mode, camera_image=args.camera_image)
    ds = SyntheticTrainDataset(cfg, args.frames, post, seed=args.seed + 7, **kw)
    val = SyntheticTrainDataset(cfg, args.val_frames, post, seed=args.seed + 100007, **kw) if args.val_frames > 0 else None
    return cfg, model, pre, post, ds, val


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--agents", type=int, default=5)
    ap.add_argument("--grid", type=int, nargs=2, default=None, metavar=("NX", "NY"),
                    help="pillar grid; default 256 x 128, or 256 x 256 with the FAX camera detector (it needs a square grid)")
    ap.add_argument("--small", action="store_true", help="PointPillar layer_nums [1, 2, 2]")
    ap.add_argument("--precision", default="f32", choices=["f32", "f16"], help="precision of the frozen encoder's kernels")
    ap.add_argument("--val_frames", type=int, default=2, help="frames of the validation split (0: no validation pass)")
    ap.add_argument("--camera_ratio", type=float, default=0.0,
                    help="camera_to_lidar_ratio of the modality roll (basedataset.py:193-200); > 0 puts the CVT lift in the camera slot")
    ap.add_argument("--ego_mode", default="mixed", choices=["mixed", "lidar", "camera"])
    ap.add_argument("--camera_image", type=int, default=64, help="camera image size of the synthetic frames")
    ap.add_argument("--train_camera_backbone", action="store_true",
                    help="do NOT freeze the camera encoder: ResNet, cross-view lift and decoder train too (hm-vit_amd/camera_train.py)")
    ap.add_argument("--train_lidar_backbone", action="store_true",
                    help="do NOT freeze the LiDAR encoder: PointPillar trains too (hm-vit_amd/encoder_train.py)")
    ap.add_argument("--model_dir", default=None, help="folder with net_epoch%%d.pth to resume from / save into")
    ap.add_argument("--stage", default="hetero", choices=["hetero", "lidar_backbone", "camera_backbone"],
                    help="lidar_backbone: stage 1, the standalone PointPillar detector on single-agent samples "
                         "(point_pillar_late_fusion.yaml); camera_backbone: stage 1, the standalone FAX camera detector on single "
                         "camera-agent samples (fax_late_fusion.yaml); hetero: the HM-ViT model (stage 2)")
    ap.add_argument("--batch", type=int, default=None,
                    help="samples per step of the stage-1 detectors (the yamls' batch_size: 8 lidar_backbone, 3 camera_backbone)")
    ap.add_argument("--lidar_backbone_dir", default=None,
                    help="folder with a stage-1 net_epoch%%d.pth: loaded into model.lidar_encoder before it is frozen")
    ap.add_argument("--camera_encoder", default="cvt", choices=["cvt", "fax"],
                    help="what fills the camera slot of stage 2: the CVT lift, or the FAX camera detector's trunk")
    ap.add_argument("--camera_backbone_dir", default=None,
                    help="folder with a --stage camera_backbone net_epoch%%d.pth: loaded into model.camera_encoder (needs "
                         "--camera_encoder fax) before it is frozen")
    ap.add_argument("--fused_loss", action="store_true",
                    help="the HIP loss kernel pair (FusedPointPillarLoss) instead of the elementwise torch loss in stage 2")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="process-group backend (nccl = RCCL)")
    ap.add_argument("--verbose", action="store_true")
    args = ap.parse_args(argv)
    if args.grid is None:
        args.grid = [256, 256] if args.stage == "camera_backbone" or args.camera_encoder == "fax" else [256, 128]
    if args.batch is None:
        args.batch = 3 if args.stage == "camera_backbone" else 8
    check_args(args)                                   # ValueError before any device work
    if not torch.cuda.is_available():
        raise SystemExit("hm-vit_amd has no CPU path: this needs an MI355X")
    info = init_distributed_mode(args.backend)
    hypes = default_hypes(args.epochs)
    stage1 = args.stage in ("lidar_backbone", "camera_backbone")
    if stage1 or args.fused_loss:
        hypes["loss"]["fused"] = True
    cfg, model, pre, post, ds, val = build(args)
    init_epoch = 0
    if args.model_dir and os.path.exists(args.model_dir):
        init_epoch, model = load_saved_model(args.model_dir, model)
    model = model.to(f"cuda:{info['gpu']}")
    res = train(model, ds, pre, hypes, saved_path=args.model_dir, init_epoch=init_epoch, dist_info=info,
                log=print if args.verbose and info["rank"] == 0 else None, val_dataset=val,
                batch_fn={"lidar_backbone": to_late_batch, "camera_backbone": to_late_camera_batch}.get(args.stage, to_batch))
    if info["rank"] == 0:
        res.update(agents=args.agents, grid=args.grid, frames=args.frames, stage=args.stage)
        if stage1:
            res.update(batch=args.batch)
        print(json.dumps(res))
    if info["distributed"]:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
