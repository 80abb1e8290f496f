#!/usr/bin/env python3
"""Headline benchmark: fused 5-agent BEV scenes/s of the HM-ViT fusion hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W            (N > 1: this process spawns the N ranks itself)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
    python bench.py ... --dump-outputs DIR                  (+ what the last timed step returned, as DIR/<name>.npy)

A "step" is one HeteroFusion forward (bevformer_point_pillar_hetero.py:39-49) on one synthetic
scene of BASELINE.json configs[1]: 5 LiDAR agents, 200x704 BEV, C=256, window 8, 2 iterations,
poses / metres-per-pixel of SURVEY.md 8(d).  Inputs are resident in HBM before the timed region.
Scenes shard one-per-GPU with no data-path collective (inference): every rank runs its own
scene, `value` = scenes processed by all ranks / max-over-ranks wall time ("weak" scaling).

Precision modes (--precision; the headline is the one at the reference's precision):
  split  (default) every fp32 product on the f16 matrix pipes as x = hi + lo (two f16 halves per operand, three MFMA
         products per fp32 product, f32 accumulate): held to the fp32 tolerance 1e-4 by tests/test_hip_fusion.py
  mixed  split-operand chains, attention operands Q / K' / V' / O stored and multiplied as f16 (C = 256 only); 1e-4 on the
         parity cases, reported under "mixed_a16"
  f32    exact-f32 MFMA (v_mfma_f32_32x32x2_f32), tolerance 1e-4
  f16    f16 operands, f32 accumulate / softmax / LayerNorm / residual: north_star's 1e-3 tolerance mode, reported
         on the same line under "fast_f16" -- narrower than the reference's fp32, so never the headline.

Rank 0 prints ONE JSON line.  Besides the contract fields it carries
  roofline      the dominant kernel of the headline mode (by HIP-event time inside this process) against the roof that binds
                it: the split-mode attention is HBM-bound (f32 planes), so it is stated in algorithmic GB/s against 8 TB/s with
                north_star's MFMA framing as `mfma_view`; the f16 / mixed kernels keep the MFMA framing (+ `hbm_view`),
  cpu_baseline  the CPU oracle (oracle/hmvit_oracle.py, PyTorch-CPU fp32 restatement of the
                reference) timed on the host cores on a bounded crop of the same workload, best thread count of a sweep,
  phases        per-phase milliseconds of one forward (HIP events on the launch stream),
  fast_f16      value / ms_per_step / roofline / phases of the f16-operand mode (1e-3 tolerance),
  mixed_a16     the same for the "mixed" mode: split-operand fp32 Linear / FFN chains, f16 attention operands (1e-4 on
                every parity case, but input-dependent -- a side figure),
  strict_f32    scenes/s of the exact-f32 MFMA mode,
  train_step    milliseconds of one training step of the fusion (forward with dropout + backward + AdamW) on the same scene,
  encoders      the two BEV encoders north_star names beside the fusion, at the shipped size (5 agents; 20 k pillars on a
                512 x 512 grid -> PointPillar -> (5, 256, 128, 128); 4 cameras of 512 x 512 per agent -> ResNet-34 + CVT lift ->
                the same): ms per 5-agent call, algorithmic TFLOP/s of their convolutions against the f16 MFMA peak,
  model_e2e     pillars + images -> psm / rm of the whole hetero model (agent types 10110) at the shipped 128 x 128 BEV size,
  other_configs fusion scenes/s of the remaining BASELINE configs (cfg1 / cfg3 / cfg4) and the shipped 128 x 128 size,
  dense_masked_tiles  scenes/s with skip_masked off: `value` skips (ego, source, window) key tiles in which every key
                is masked (outside the source's field of view) and windows of non-ego agents whose results cannot
                reach ego 0's output row; this is the same forward without those two shortcuts.
"""
import argparse
import contextlib
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CONFIGS = {
    # name: (L, C, H, W, window, modes, voxel, downsample)
    "cfg1": dict(L=2, C=64, H=100, W=352, window=4, modes=[1, 1], voxel=0.4, downsample=2),
    "cfg2": dict(L=5, C=256, H=200, W=704, window=8, modes=[1, 1, 1, 1, 1], voxel=0.4, downsample=1),
    "cfg3": dict(L=5, C=256, H=200, W=704, window=8, modes=[1, 0, 1, 1, 0], voxel=0.4, downsample=1),
    "cfg4": dict(L=5, C=256, H=200, W=704, window=8, modes=[0, 0, 0, 0, 0], voxel=0.4, downsample=1),
    "native": dict(L=5, C=256, H=128, W=128, window=8, modes=[1, 0, 1, 1, 0], voxel=0.4, downsample=4),
}
# dense MFMA TFLOP/s (MI355X_MICROARCH.md).  The split mode runs on the f16 pipes: its roof is the f16 peak, its
# numerator stays the ALGORITHMIC (fp32-product) flop count -- the three-fold MFMA work is overhead, not credit.
PEAK = {"f16": 2500.0, "split": 2500.0, "mixed": 2500.0, "f32": 157.3}
PEAK_HBM = 8000.0                          # GB/s
DTYPE = {
    "f16": "f16 operands, f32 accumulate/softmax/LayerNorm/residual (1e-3 tolerance mode)",
    "split": "fp32 via split f16 operands (x = hi + lo, 3 MFMA products per fp32 product), f32 accumulate/softmax/LayerNorm/residual",
    "mixed": "fp32 via split f16 operands (3 MFMA products per fp32 product) in every Linear / FFN / LayerNorm / residual; attention "
             "operands Q / K' / V' / O stored and multiplied as f16 (f32 accumulate / softmax)",
    "f32": "f32 (exact-f32 MFMA)",
}
TOLERANCE = {"f16": 1e-3, "split": 1e-4, "mixed": 1e-4, "f32": 1e-4}
ES = {"f16": 2, "split": 4, "mixed": 2, "f32": 4}      # bytes per stored activation element (Q / K' / V' / O planes)
DUMP_BYTES = 32 * 2 ** 20                  # --dump-outputs: data bytes of all arrays together (half the 64 MB allowance)


def dump_outputs(out_dir, arrays):
    """`--dump-outputs DIR`: the arrays the timed path returned in its last step, as DIR/<name>.npy in float32 (float64 stays
    float64), so that two builds can be compared output for output on the same seeded inputs.  Each array gets an equal share of
    DUMP_BYTES; one larger than its share is written as a sample: the elements of its flattened form at indices drawn without
    replacement by numpy.random.default_rng(0), in ascending order - the same indices in every run of the same shape.  The inference
    forward is bit-reproducible; a --train dump is not (float atomics in the backward pass, amplified by AdamW): compare it to a tolerance.
    Returns what was written, per array, for the result line."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for name, t in arrays.items():
        a = t.detach().cpu().numpy()
        a = a.astype(np.float64 if a.dtype == np.float64 else np.float32)
        info = {"shape": list(a.shape), "dtype": str(a.dtype)}
        keep = DUMP_BYTES // len(arrays) // a.itemsize
        if a.size > keep:
            info["sampled_elements"] = keep
            a = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, keep, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)
        written[name] = info
    return written


def phase_work(c, num_iters, es):
    """Algorithmic FLOPs (MFMA phases) or bytes (HBM phases) of ONE launch of each phase for a
    full (un-pruned) stage, and of the pruned last stage; SURVEY.md 8(d) formulas."""
    L, C, P = c["L"], c["C"], c["H"] * c["W"]
    n = c["window"] ** 2
    mlp = C
    E = len(set(c["modes"]))

    def stage(n_ego, n_ffn, e):
        return {
            "ln_attn": ("hbm", L * P * C * (4 + es)),
            "qkv_gemm": ("mfma", 2 * P * C * C * n_ego + 2 * P * 2 * C * C * L * e),
            "attention": ("mfma", 2 * 2 * n_ego * P * (L * n) * C),
            "out_proj": ("mfma", 2 * P * C * C * n_ego),
            "ln_ffn": ("hbm", n_ffn * P * C * (4 + es)),
            "ffn1": ("mfma", 2 * P * C * mlp * n_ffn),
            "ffn2": ("mfma", 2 * P * C * mlp * n_ffn),
        }
    full, last = stage(L, L, E), stage(1, 1, 1)
    n_stages = 2 * num_iters
    out = {}
    for k in full:
        kind, w_full = full[k]
        out[k] = (kind, (w_full * (n_stages - 1) + last[k][1]) / n_stages)   # mean per launch
    out["head"] = ("mfma", 2 * 2 * P * C * C)
    out["_full"], out["_last"] = full, last            # per-stage figures (the fused launches are not one phase of one stage each)
    out["layout_in"] = ("hbm", L * P * C * 8)
    out["layout_out"] = ("hbm", P * C * 8)
    return out


def kernel_source_hash():
    """sha256 over the HIP sources: stamps profiles/pmc_traffic.json so that a stale PMC figure is never attached to a
    bench line of different kernels (there is no .git on the GPU box)."""
    h = hashlib.sha256()
    d = os.path.join(ROOT, "hm-vit_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".hpp")):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def cpu_baseline(cfgd, num_iters, seed):
    """The oracle timed on the host cores on a crop of the workload (same agents, channels, window and poses; 40x176 pixels
    instead of 200x704), scaled to full scenes by pixel count -- the reference's cost is linear in the number of windows.
    Thread count: a short ascending sweep on a smaller crop (8 / 16 / 32 / 64 / all, stopped once a count is 1.5x slower than the
    best so far - an oversubscribed torch is slower than the reference's own 8-core figure); the sample is then timed at the best."""
    import torch
    from oracle import hmvit_oracle as O
    big = cfgd["H"] * cfgd["W"] > 40 * 176
    Hs, Ws = (40, 176) if big else (cfgd["H"], cfgd["W"])
    cfg = O.make_config(cfgd["C"], cfgd["window"], cfgd["L"], voxel=cfgd["voxel"],
                        downsample=cfgd["downsample"], num_iters=num_iters)
    sd = O.random_state_dict(cfg, seed=0)
    ncpu = os.cpu_count() or 8
    default_threads = torch.get_num_threads()
    sweep = {}
    if big:
        small = O.synthetic_scene(cfgd["L"], cfgd["C"], 16, 88, cfgd["modes"], seed=seed)
        for nt in sorted({t for t in (8, 16, 32, 64, ncpu) if t <= ncpu}):
            torch.set_num_threads(nt)
            O.hetero_fusion(*small, sd, cfg)
            t0 = time.perf_counter()
            O.hetero_fusion(*small, sd, cfg)
            sweep[nt] = time.perf_counter() - t0
            if sweep[nt] > 1.5 * min(sweep.values()):
                break        # past the optimum: larger counts only oversubscribe (all 256 host threads: 140 s per forward)
        best = min(sweep, key=sweep.get)
    else:
        best = min(default_threads, ncpu)
    torch.set_num_threads(best)
    scene = O.synthetic_scene(cfgd["L"], cfgd["C"], Hs, Ws, cfgd["modes"], seed=seed)
    O.hetero_fusion(*scene, sd, cfg)                     # warm-up
    reps, t0 = 0, time.perf_counter()
    while True:
        O.hetero_fusion(*scene, sd, cfg)
        reps += 1
        dt = time.perf_counter() - t0
        if dt > 12.0 or reps >= 5:
            break
    torch.set_num_threads(default_threads)
    frac = (Hs * Ws) / float(cfgd["H"] * cfgd["W"])
    return {"value": reps / dt * frac, "unit": "scenes/s", "cores": best, "kind": "port",
            "sample": f"{reps} forward(s) of the CPU oracle on a {Hs}x{Ws} crop ({frac * 100:.1f}% of the "
                      f"{cfgd['H']}x{cfgd['W']} scene's windows), {dt / reps:.2f} s each at {best} threads, scaled by pixel count",
            "thread_sweep_s": {str(k): round(v, 3) for k, v in sweep.items()},
            "full_size_check": "one full-size forward on the same host class (profiles/r05_cpu_full.txt, `bench.py --cpu-baseline-full`): "
                               "82.6 s at 16 threads = 0.0121 scenes/s = 1.056 x this crop estimate",
            "reference_itself": "the reference's own HeteroFusion.forward measured in the build container on 8 cores: "
                                "122.8 s/scene = 0.0081 scenes/s at cfg2 (BASELINE.md section 2)"}


def cpu_baseline_full(cfgd, num_iters, seed, threads):
    """ONE forward of the CPU oracle at the FULL size of the workload on the host cores of this box (BASELINE.md section 4 /
    SURVEY 8d: "1 + 1 for cfg2"), printed with the thread count and the CPU model string, and - next to it - the same crop
    measurement the default bench line carries, so that the pixel-count scaling of `cpu_baseline` can be checked against a
    real full-size run.  Minutes of CPU: `python bench.py --cpu-baseline-full` is a separate invocation, never part of the
    driver's command.  The committed record is profiles/r05_cpu_full.txt."""
    import platform
    import torch
    from oracle import hmvit_oracle as O
    cfg = O.make_config(cfgd["C"], cfgd["window"], cfgd["L"], voxel=cfgd["voxel"], downsample=cfgd["downsample"], num_iters=num_iters)
    sd = O.random_state_dict(cfg, seed=0)
    model = platform.processor() or "?"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    crop = cpu_baseline(cfgd, num_iters, seed)
    nt = threads or crop["cores"]
    torch.set_num_threads(nt)
    scene = O.synthetic_scene(cfgd["L"], cfgd["C"], cfgd["H"], cfgd["W"], cfgd["modes"], seed=seed)
    t0 = time.perf_counter()
    with torch.no_grad():
        y = O.hetero_fusion(*scene, sd, cfg)
    dt = time.perf_counter() - t0
    full = 1.0 / dt
    return {"workload": f"{cfgd['L']} agents {cfgd['H']}x{cfgd['W']} C={cfgd['C']} window {cfgd['window']}, {num_iters} iterations: one full-size "
                        "forward of oracle/hmvit_oracle.py (cold: no warm-up run at this size)",
            "seconds": round(dt, 2), "scenes_per_s": full, "threads": nt, "host_cpus": os.cpu_count(), "cpu_model": model,
            "output_checksum": float(y.double().abs().mean()),
            "crop_estimate": crop, "full_over_crop_estimate": full / crop["value"]}


def _time_ms(fn, n, warmup, reps=3):
    """ms per call of the side figures: median over `reps` batches of `n` back-to-back calls (HIP events around a batch).  The
    encoder / model paths are a hundred launches per call from Python, so one host hiccup on a shared box moves a single batch by
    20-100 % (round 4: 2.9 against 6.7 ms for the same PointPillar call); the median of three batches does not see it."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    batches = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        batches.append(e0.elapsed_time(e1) / n)
    return sorted(batches)[len(batches) // 2]


def other_configs(args, dev, precision, hmvit_amd, S):
    """Fusion scenes/s of the BASELINE configs that are not the headline (and the shipped 128 x 128 size), same precision mode."""
    import torch
    out = {}
    for name, cc in CONFIGS.items():
        if name == args.config or (precision == "mixed" and cc["C"] != 256):
            continue
        cfg = S.make_config(cc["C"], cc["window"], cc["L"], voxel=cc["voxel"], downsample=cc["downsample"], num_iters=args.num_iters)
        net = S.seeded_fusion(cfg, precision=precision, seed=0).to(dev).eval()
        scene = [t.to(dev) for t in S.synthetic_scene(cc["L"], cc["C"], cc["H"], cc["W"], cc["modes"], seed=1)]
        with torch.no_grad():
            ms = _time_ms(lambda: net(*scene), 10, 2)
        out[name] = {"value": 1e3 / ms, "unit": "scenes/s", "ms_per_step": ms,
                     "workload": f"{cc['L']} agents modes {''.join(map(str, cc['modes']))}, {cc['H']}x{cc['W']}, C={cc['C']}, window {cc['window']}"}
        del net, scene
        torch.cuda.empty_cache()
    return out


def encoder_lines(dev, precision, hmvit_amd, S):
    """north_star's BEV encoders and the whole hetero model at the shipped size.  Random-init weights
    (the modules' own default initialisation), synthetic pillars / images; times from HIP events around `n` calls."""
    import torch
    from hmvit_amd import replay as R
    from hmvit_amd.camera import CvtCameraEncoder
    L, nx, ny, image = 5, 512, 512, 512
    mcfg = R.lidar_model_config(nx, ny, max_cav=L)
    torch.manual_seed(0)
    vf, vc, vn = S.synthetic_pillars(L, 20000, nx, ny, mcfg["lidar"], seed=2)
    lidar_batch = {"processed_lidar": {"voxel_features": vf.to(dev), "voxel_coords": vc.to(dev), "voxel_num_points": vn.to(dev)},
                   "record_len": torch.tensor([L]), "n_agents": L}    # (the assembled model passes the count too: no read-back per call)
    ccfg = S.camera_config(image=image, num_layers=34, bev_h=256, bev_w=256)
    cams = {k: v.to(dev) for k, v in S.synthetic_cameras(L, image, seed=8).items()}
    enc = {}
    with torch.no_grad():
        pp = hmvit_amd.PointPillar(mcfg["lidar"], precision=precision).to(dev).eval()
        pp.set_return_features()
        ms = _time_ms(lambda: pp(lidar_batch), 10, 4)
        tf = 0.1436 * L                                   # 143.6 GFLOP of convolutions per agent (20 k pillars)
        enc["pointpillar"] = {"ms": ms, "algorithmic_TFLOP": tf, "achieved_TFLOPs": tf / (ms * 1e-3), "peak_TFLOPs": PEAK[precision],
                              "frac": tf / (ms * 1e-3) / PEAK[precision], "traffic": None,
                              "workload": "5 agents x 20 k pillars, 512x512 grid, layers [3, 5, 8] -> (5, 256, 128, 128)"}
        del pp
        cam = CvtCameraEncoder(ccfg, precision=precision).to(dev).eval()
        ms = _time_ms(lambda: cam(cams), 5, 2)
        tf = S.resnet_trunk_flops(34, image) * 4 * L / 1e12
        enc["cvt"] = {"ms": ms, "algorithmic_TFLOP": tf, "achieved_TFLOPs": tf / (ms * 1e-3), "peak_TFLOPs": PEAK[precision],
                      "frac": tf / (ms * 1e-3) / PEAK[precision], "traffic": None,
                      "workload": "5 agents x 4 cameras of 512x512, ResNet-34 trunk (the priced flops) + cross-view lift (32x32 queries, "
                                  "16384 + 1024 keys) + decoder -> (5, 256, 128, 128)"}
        # whole hetero model: BASELINE configs[2]'s agent types, every agent carries both sensors' inputs and `mode` picks one
        _, pw, _, _, _ = S.synthetic_scene(L, 1, 1, 1, [1] * L, seed=0)
        batch = dict(lidar_batch)
        batch.update({"mode": torch.tensor([[1.0, 0.0, 1.0, 1.0, 0.0]], dtype=torch.float64), "pairwise_t_matrix": pw.to(dev)})
        batch.update(cams)
        net = hmvit_amd.BevformerPointPillarHetero(mcfg, camera_encoder=cam, precision=precision).to(dev).eval()
        ms = _time_ms(lambda: net(batch), 5, 2)
        # per-module split of the same forward: HIP events from forward hooks around the four sub-modules,
        # median over 5 forwards; "other" = regroup, the interleave of camera / LiDAR maps, the small-input read-back
        mods = {"camera_encoder": net.camera_encoder, "lidar_encoder": net.lidar_encoder, "fusion_net": net.fusion_net, "decoder": net.decoder}
        marks, hooks = {}, []
        for name, m in mods.items():
            def pre(_m, _i, name=name):
                e = torch.cuda.Event(enable_timing=True); e.record(); marks.setdefault(name, []).append([e, None])
            def post(_m, _i, _o, name=name):
                e = torch.cuda.Event(enable_timing=True); e.record(); marks[name][-1][1] = e
            hooks += [m.register_forward_pre_hook(pre), m.register_forward_hook(post)]
        for _ in range(5):
            net(batch)
        torch.cuda.synchronize()
        for h in hooks:
            h.remove()
        split = {k: sorted(a.elapsed_time(b) for a, b in v)[len(v) // 2] for k, v in marks.items()}
        split["other"] = max(0.0, ms - sum(split.values()))
        e2e = {"ms_per_scene": ms, "value": 1e3 / ms, "unit": "scenes/s", "precision": precision,
               "modules_ms": {k: round(v, 3) for k, v in split.items()},
               "workload": "5 agents 10110 (2 camera + 3 LiDAR): pillars + images -> PointPillar / ResNet-34 + CVT -> HeteroFusion "
                           "(128x128, C=256, window 8, 2 iters) -> HeteroDecoder -> psm / rm; random-init weights"}
        del net, cam
    torch.cuda.empty_cache()
    # HBM bytes per forward from the PMC passes of the same sources (tools/probe/r04_encoder_traffic.sh), null when the sources changed
    tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    if precision == "split" and os.path.exists(tpath):
        tj = json.load(open(tpath))
        if tj.get("kernel_source_hash") == kernel_source_hash():
            for k, v in tj.get("encoders_split", {}).items():
                if k in enc:
                    enc[k]["traffic"] = v
    return enc, e2e


def train_bench(args, c, dev, rank, world, scene, make, barrier, D):
    """`--train`: the per-rank train step of train_camera.py:163-199 on the fusion (the hot path): every rank holds its own
    scene, the model is wrapped in DistributedDataParallel(find_unused_parameters=True) as train_camera.py:126-131 does, and the
    only exchange of a step is DDP's bucketed gradient all-reduce (RCCL over xGMI with --backend nccl).  Timed like the
    inference line (barrier + synchronise on both sides, max over ranks); besides ms_per_step the line carries the same step
    without the exchange (`no_sync`), their difference (the all-reduce time that backward does not hide) and a stand-alone
    all-reduce of one gradient-sized buffer."""
    import torch
    import torch.distributed as dist
    if args.stub:
        class Stub(torch.nn.Module):           # CPU stand-in with an unused parameter (find_unused_parameters must cope)
            def __init__(self):
                super().__init__()
                self.a, self.unused = torch.nn.Linear(64, 64), torch.nn.Linear(8, 8)

            def forward(self, *_):
                return self.a(torch.ones(4, 64))
        torch.manual_seed(0)
        net = Stub()
        opt = torch.optim.AdamW(net.parameters(), lr=1e-3)
        target = torch.zeros(4, 64)
    else:
        from hmvit_amd import train as T
        net = make("f32").train()
        net.train_recompute = args.train_recompute
        opt = T.make_optimizer(net.parameters())
        target = torch.zeros(1, c["C"], c["H"], c["W"], device=dev)
    model = net
    if world > 1:
        model = torch.nn.parallel.DistributedDataParallel(net, device_ids=None if args.stub else [dev.index],
                                                          find_unused_parameters=True)

    def step(sync_grads=True):
        opt.zero_grad()
        with model.no_sync() if world > 1 and not sync_grads else contextlib.nullcontext():
            y = model(*scene)
            loss = (y - target).pow(2).mean()
            loss.backward()
        opt.step()
        return y.detach(), loss.detach()

    def timed(n, sync_grads):
        barrier()
        t0 = time.perf_counter()
        for _ in range(n - 1):
            step(sync_grads)
        last = step(sync_grads)
        barrier()
        return D.max_over_ranks(time.perf_counter() - t0, dev), last

    for _ in range(max(1, args.warmup)):
        step()
    dt, last = timed(args.steps, True)
    dumped = None
    if args.dump_outputs and rank == 0:
        dumped = dump_outputs(args.dump_outputs, {"fusion_out": last[0], "loss": last[1]})
    del last
    dt_local = timed(args.steps, False)[0] if world > 1 else dt
    n_grad = sum(p.numel() for p in net.parameters() if p.grad is not None)
    ar_ms = None
    if world > 1:
        buf = torch.zeros(max(1, n_grad), device=dev)
        dist.all_reduce(buf)
        barrier()
        t0 = time.perf_counter()
        for _ in range(5):
            dist.all_reduce(buf)
        barrier()
        ar_ms = D.max_over_ranks(time.perf_counter() - t0, dev) / 5 * 1e3
    units = D.sum_over_ranks(float(args.steps), dev)
    res = {"metric": "train steps/sec (HeteroFusion forward + backward + gradient all-reduce + AdamW, one scene per rank)",
           "value": units / dt, "unit": "steps/s", "n_gpus": world, "steps": args.steps, "warmup": max(1, args.warmup),
           "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
           "dtype": "stub" if args.stub else "f32 master weights; exact-f32 / split-f16 training kernels", "data": "stub" if args.stub else "synthetic",
           "config": {"workload": "stub" if args.stub else f"{args.config}: train step of the fusion on one scene per rank, dropout 0.1, AdamW"
                                   + (f", recompute bits {args.train_recompute}" if args.train_recompute else ""),
                      "parallelism": f"dp{world}: DistributedDataParallel(find_unused_parameters=True), backend {args.backend}"},
           "ms_per_step_no_sync": dt_local / args.steps * 1e3,
           "allreduce_exposed_ms": max(0.0, (dt - dt_local) / args.steps * 1e3),
           "allreduce_standalone_ms": ar_ms, "gradient_bytes": 4 * n_grad}
    if dumped is not None:
        res["dump_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}
    if not args.stub:
        res["peak_memory_GiB"] = torch.cuda.max_memory_allocated(dev) / 2 ** 30
    return res


def spawn_ranks(args, argv):
    """`python bench.py --gpus N` without a launcher: start the N ranks as fresh child processes BEFORE anything in this
    process touches the GPU (a process that has initialised HIP must never exec), forward rank 0's stdout, return the worst
    exit code.  Same environment contract as torch.distributed.run (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ)
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + argv, env=env,
                                      stdout=subprocess.PIPE if r == 0 else subprocess.DEVNULL))
    out, _ = procs[0].communicate()
    rc = procs[0].returncode
    for p in procs[1:]:
        rc = max(rc, p.wait())
    sys.stdout.write(out.decode())
    sys.stdout.flush()
    return rc


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="cfg2", choices=sorted(CONFIGS))
    ap.add_argument("--precision", default=None, choices=["split", "mixed", "f32", "f16"])
    ap.add_argument("--num-iters", type=int, default=2)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-strict", action="store_true", help="skip the side figures (fast_f16, strict_f32, dense_masked_tiles)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="gloo + --stub: CPU test of the launch logic")
    ap.add_argument("--stub", action="store_true", help="replace the forward by a CPU stand-in (tests/test_dist_cpu.py)")
    ap.add_argument("--cpu-baseline-full", action="store_true",
                    help="one FULL-size forward of the CPU oracle on the host cores (minutes; no GPU work; not the driver's command)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="threads of --cpu-baseline-full (default: the crop sweep's best)")
    ap.add_argument("--train-recompute", type=int, default=0, choices=(0, 1, 3),
                    help="--train: HmvitFusionTrainDesc::recompute bits (1: the FFN pre-activations, 3: + the queries are recomputed in the "
                         "backward pass instead of kept: cfg2 peak 32.8 -> 30.1 -> 27.4 GiB for +1.6 / +4.0 ms per step, cumulative)")
    ap.add_argument("--train", action="store_true",
                    help="the training half of north_star instead of the inference headline: one DistributedDataParallel train step "
                         "per rank (HeteroFusion forward with dropout + HIP backward + gradient all-reduce on RCCL + AdamW)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what rank 0's last timed step returned as DIR/<name>.npy (float32; a larger "
                         "output as a fixed seeded sample, at most 32 MiB in all): the forward's fused map, with --train also the loss")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    if args.cpu_baseline_full:
        print(json.dumps(cpu_baseline_full(CONFIGS[args.config], args.num_iters, 1, args.cpu_threads)), flush=True)
        return
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args, argv))

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    args.gpus = world                                   # under a launcher the launcher's world size is the truth
    import torch.distributed as dist
    if args.stub:
        dev = torch.device("cpu")
    else:
        # one GPU per rank; on a box with fewer GPUs than ranks (the 1-GPU rehearsal `--gpus 2 --backend gloo`) ranks share devices
        local_dev = local_rank % max(1, torch.cuda.device_count())
        torch.cuda.set_device(local_dev)
        dev = torch.device("cuda", local_dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)   # "nccl" is RCCL on ROCm
        else:
            dist.init_process_group(backend="gloo")

    def sync():
        if dev.type == "cuda":
            torch.cuda.synchronize(dev)

    def barrier():
        sync()
        if world > 1:
            dist.barrier()
        sync()

    c = CONFIGS[args.config]
    if args.stub:
        from importlib import util as _u
        spec = _u.spec_from_file_location("hmvit_dist", os.path.join(ROOT, "hm-vit_amd", "dist.py"))
        D = _u.module_from_spec(spec)
        spec.loader.exec_module(D)
        precision = "stub"
        a = torch.randn(64, 64, generator=torch.Generator().manual_seed(0))

        def make(_):
            return lambda *s: (a @ a).sum()
        scene = []
    else:
        import hmvit_amd
        from hmvit_amd import dist as D
        from hmvit_amd import synthetic as S      # seeded workload generators (the oracle is only the cpu_baseline leg)
        precision = args.precision or hmvit_amd.REFERENCE_PRECISION
        cfg = S.make_config(c["C"], c["window"], c["L"], voxel=c["voxel"], downsample=c["downsample"],
                            num_iters=args.num_iters)
        # every rank gets its own scene (different features, same geometry)
        scene = [t.to(dev) for t in S.synthetic_scene(c["L"], c["C"], c["H"], c["W"], c["modes"], seed=1 + rank)]

        def make(prec):
            return S.seeded_fusion(cfg, precision=prec, seed=0).to(dev).eval()

    def timed(net, steps, warmup):
        with torch.no_grad():
            for _ in range(warmup):
                net(*scene)
            barrier()
            t0 = time.perf_counter()
            for _ in range(steps - 1):
                net(*scene)
            last = net(*scene)              # what the last step returned (--dump-outputs)
            barrier()
        dt = time.perf_counter() - t0
        # job time = slowest rank; units = what all ranks processed (hm-vit_amd/dist.py)
        return D.max_over_ranks(dt, dev), D.sum_over_ranks(float(steps), dev), last

    if args.train:
        result = train_bench(args, c, dev, rank, world, scene, make, barrier, D)
        if rank == 0:
            print(json.dumps(result), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    net = make(precision)
    dt, units, last = timed(net, args.steps, args.warmup)
    value = units / dt
    dumped = dump_outputs(args.dump_outputs, {"fusion_out": last}) if args.dump_outputs and rank == 0 else None
    del last

    result = {
        "metric": "fused BEV scenes/sec (5 agents, 200x704 BEV, C=256)" if args.config == "cfg2"
                  else f"fused BEV scenes/sec ({args.config})",
        "value": value, "unit": "scenes/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None,
        "dtype": DTYPE.get(precision, precision),
        "data": "synthetic",
        "config": {"workload": f"{args.config}: {c['L']} agents modes {''.join(map(str, c['modes']))}, "
                               f"{c['H']}x{c['W']} BEV, C={c['C']}, window {c['window']}, "
                               f"{args.num_iters} iters, {c['voxel'] * c['downsample']:.1f} m/px; "
                               "HeteroFusion.forward, inputs resident in HBM",
                   "parallelism": f"{world} independent scene replica(s), no data-path collective",
                   "tolerance": f"{TOLERANCE.get(precision, 0):g} rel-max vs the reference's fp32 forward (tests/test_hip_fusion.py, "
                                "goldens g12 / g13 at this size)",
                   "masked_tiles": "exact dead-work elimination (identical output): key tiles whose 64 keys are all masked "
                                   "are skipped, and so are windows of non-ego agents that ego 0 - the only row "
                                   "HeteroFusion returns - cannot reach in the last two stages; figure with both off in "
                                   "dense_masked_tiles"},
    }
    if args.stub:
        result["config"] = {"workload": "stub (CPU stand-in: launch / barrier / reduction logic only)",
                            "parallelism": f"{world} ranks, backend {args.backend}"}
        result["data"] = "stub"
    if dumped is not None:
        result["dump_outputs"] = {"dir": args.dump_outputs, "arrays": dumped}

    def roofline_of(net, prec):
        """Per-phase HIP-event times of one forward on the launch stream (median of 5), the dominant phase's roofline."""
        runs = [net.profile_phases(*scene) for _ in range(5)]
        es = ES[prec]
        work = phase_work(c, args.num_iters, es)
        full_st, last_st = work.pop("_full"), work.pop("_last")
        fused = prec in ("f16", "split", "mixed")
        rename = {"qkv_gemm": "ln_qkv", "ffn2": "stage_tail"} if fused else {}
        phases = {}
        for name in runs[0]:
            ms = sorted(r[name][0] for r in runs)[2]
            cnt = runs[0][name][1]
            if cnt:
                phases[rename.get(name, name)] = {"ms_total": round(ms, 4), "launches": cnt}
        if fused:
            # one fused kernel per stage does out-proj + LayerNorm + FFN (+ the next stage's LayerNorm + Q / K' / V'
            # projections): "stage_tail"; the first stage's LayerNorm + projections run as "ln_qkv"
            # "head" = the LAST stage's tail with mlp_head appended (one launch, ego rows): its own phase since round 6
            n_st = 2 * args.num_iters
            tail_of = lambda st_: st_["out_proj"][1] + st_["ffn1"][1] + st_["ffn2"][1]
            fused_head = phases.get("head", {}).get("ms_total", 0.0) > 0.05        # (f32 mode / old libraries: mlp_head alone, or nothing)
            if fused_head and n_st > 1:
                # n_st - 1 fused tails of full stages, each with the next stage's projections (the last of them: the pruned stage's)
                work["stage_tail"] = ("mfma", ((n_st - 1) * tail_of(full_st) + (n_st - 2) * full_st["qkv_gemm"][1] + last_st["qkv_gemm"][1]) / (n_st - 1))
                work["head"] = ("mfma", tail_of(last_st) + work["head"][1])
            else:
                work["stage_tail"] = ("mfma", work["out_proj"][1] + work["ffn1"][1] + work["ffn2"][1] +
                                      work["qkv_gemm"][1] * (n_st - 1) / n_st)
            work["ln_qkv"] = ("mfma", full_st["qkv_gemm"][1])
        dom = max(phases, key=lambda k: phases[k]["ms_total"])
        kind, per_launch = work[dom]
        avg_s = phases[dom]["ms_total"] / phases[dom]["launches"] * 1e-3
        if kind == "mfma":
            achieved, peak, unit = per_launch / avg_s / 1e12, PEAK[prec], "TFLOP/s"
        else:
            achieved, peak, unit = per_launch / avg_s / 1e9, PEAK_HBM, "GB/s"
        # HBM bytes per launch of the dominant kernel from the rocprofv3 PMC passes of the same command (FETCH_SIZE with
        # the gfx950 x2 wide-read correction + WRITE_SIZE; tools/pmc_summary.py writes profiles/pmc_traffic.json with the
        # hash of the kernel sources it was measured on).  Dropped (null) when the sources have changed since.
        traffic = None
        tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tpath) and args.config == "cfg2":
            tj = json.load(open(tpath))
            if tj.get("kernel_source_hash") == kernel_source_hash():
                traffic = tj.get(prec, {}).get(dom)
        roof = {"kernel": dom, "bound": kind, "achieved": achieved, "peak": peak, "unit": unit,
                "frac": achieved / peak, "traffic": traffic, "avg_launch_ms": avg_s * 1e3,
                "algorithmic_per_launch": per_launch}
        # where `traffic` comes from: a builder-side PMC pass over the same sources, NOT something this run observed
        tsrc = {"file": "profiles/pmc_traffic.json", "collected_by": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of `python bench.py` on a "
                "builder box (tools/probe/r06_evidence.sh, tools/pmc_summary.py); FETCH x2 (gfx950 wide-read correction) + WRITE",
                "file_kernel_source_hash": None, "this_run_kernel_source_hash": kernel_source_hash(), "match": False}
        if os.path.exists(tpath):
            tsrc["file_kernel_source_hash"] = json.load(open(tpath)).get("kernel_source_hash")
            tsrc["match"] = tsrc["file_kernel_source_hash"] == tsrc["this_run_kernel_source_hash"] and args.config == "cfg2"
        roof["traffic_source"] = tsrc
        if dom == "attention":
            # the same kernel against the HBM roof: compulsory bytes = Q in + every K'/V' map once + O out, for the (ego, window)
            # items each launch actually RAN (hmvit_fusion_profile_items: the reachability pruning drops a quarter of the third
            # stage's items and four fifths of the last one's) - mean over the launches
            L_, C_, P_ = c["L"], c["C"], c["H"] * c["W"]
            n_st = 2 * args.num_iters
            items = getattr(net, "last_attention_items", None) or []
            n_win = P_ // (c["window"] ** 2)
            if len(items) == n_st:
                q_rows = [live / n_win * P_ for live, _ in items]            # query rows (= output rows) of each launch
            else:
                q_rows = [L_ * P_] * (n_st - 1) + [P_]
            comp = sum(r * C_ * es * 2 + L_ * 2 * P_ * C_ * es for r in q_rows) / n_st
            if kind == "mfma":
                per_launch = sum(2 * 2 * r * (L_ * c["window"] ** 2) * C_ for r in q_rows) / n_st
                achieved = per_launch / avg_s / 1e12
                roof.update({"achieved": achieved, "frac": achieved / peak, "algorithmic_per_launch": per_launch})
            roof["items_run_per_launch"] = [int(live) for live, _ in items] or None
            hbm = {"algorithmic_bytes_per_launch": comp, "achieved_GBps": comp / avg_s / 1e9,
                   "peak_GBps": PEAK_HBM, "frac": comp / avg_s / 1e9 / PEAK_HBM}
            if prec == "split":
                # f32 planes: this kernel's binding roof is HBM (it moves `traffic` bytes per launch at ~55 % of the HBM peak
                # with its matrix pipe ~5 % busy), so the roofline object is stated against HBM with the algorithmic bytes
                # (every K' / V' map counted ONCE, although each of the L egos gathers it through its own transform);
                # north_star's MFMA framing of the attention block rides along as mfma_view
                mfma = {"algorithmic_flops_per_launch": per_launch, "achieved_TFLOPs": achieved, "peak_TFLOPs": peak, "frac": achieved / peak}
                roof.update({"bound": "hbm", "achieved": hbm["achieved_GBps"], "peak": PEAK_HBM, "unit": "GB/s", "frac": hbm["frac"],
                             "algorithmic_per_launch": comp, "mfma_view": mfma})
            else:
                roof["hbm_view"] = hbm
                roof["mfma_view"] = {"algorithmic_flops_per_launch": per_launch, "achieved_TFLOPs": achieved, "peak_TFLOPs": peak, "frac": achieved / peak}
        # ---- every phase against both roofs: algorithmic flops and compulsory bytes of the MEAN launch of the phase,
        # its measured average launch time, and the PMC traffic of the same kernel where the committed pass matches these sources ----
        if fused:
            L_, C_, P_ = c["L"], c["C"], c["H"] * c["W"]
            n_st = 2 * args.num_iters
            E_ = len(set(c["modes"]))
            plane = P_ * C_
            items = getattr(net, "last_attention_items", None) or []
            n_win = P_ // (c["window"] ** 2)
            q_rows = [live / n_win * P_ for live, _ in items] if len(items) == n_st else [L_ * P_] * (n_st - 1) + [P_]
            by = {}
            # first stage's LayerNorm + projections: the NCHW input once, Q / K' / V' planes out
            by["ln_qkv"] = (work["ln_qkv"][1], L_ * plane * 4 + (L_ + 2 * L_ * E_) * plane * es)
            # attention: Q rows in + every K' / V' map once + O rows out, for the items each launch ran; flops on the same rows
            by["attention"] = (sum(2 * 2 * r * (L_ * c["window"] ** 2) * C_ for r in q_rows) / n_st,
                               sum(r * C_ * es * 2 + L_ * 2 * plane * es for r in q_rows) / n_st)
            # stage tails: O + residual stream in, residual stream out, the next stage's Q / K' / V' out (ego 0's Q only in front of the pruned
            # last stage); the last launch is tail + mlp_head on ego 0's rows with the NCHW map out
            tail_bytes = 0.0
            for st in range(n_st - 1):
                n_q = 1 if st == n_st - 2 else L_
                tail_bytes += L_ * plane * (es + 4 + 4) + (n_q + 2 * L_ * E_) * plane * es
            head_bytes = plane * (es + 4 + 4)
            if fused_head and n_st > 1:
                by["stage_tail"] = (work["stage_tail"][1], tail_bytes / (n_st - 1))
                by["head"] = (work["head"][1], head_bytes)
            else:
                by["stage_tail"] = (work["stage_tail"][1] + work["head"][1] / n_st, (tail_bytes + head_bytes) / n_st)
            tj = json.load(open(tpath)) if os.path.exists(tpath) else {}
            t_ok = tj.get("kernel_source_hash") == kernel_source_hash() and args.config == "cfg2"
            rbp = {}
            for name, (flops, nbytes) in by.items():
                if name not in phases:
                    continue
                t_s = phases[name]["ms_total"] / phases[name]["launches"] * 1e-3
                tr = tj.get(prec, {}).get("stage_tail_head" if name == "head" else name) if t_ok else None
                if name == "stage_tail" and "head" not in by and t_ok and tr is not None and tj.get(prec, {}).get("stage_tail_head") is not None:
                    # the file keeps the three fused tails and the tail + head launch apart: mean over the launches of the phase
                    tr = (tr * (n_st - 1) + tj[prec]["stage_tail_head"]) / n_st
                rbp[name] = {"launches": phases[name]["launches"], "avg_launch_ms": t_s * 1e3,
                             "mfma": {"algorithmic_flops_per_launch": flops, "achieved_TFLOPs": flops / t_s / 1e12, "peak_TFLOPs": PEAK[prec],
                                      "frac": flops / t_s / 1e12 / PEAK[prec]},
                             "hbm": {"algorithmic_bytes_per_launch": nbytes, "achieved_GBps": nbytes / t_s / 1e9, "peak_GBps": PEAK_HBM,
                                     "frac": nbytes / t_s / 1e9 / PEAK_HBM},
                             "traffic": tr, "traffic_over_algorithmic": (tr / nbytes) if tr else None}
            roof["by_phase"] = rbp
            if dom in rbp:      # whichever roof `roofline` is stated against, the other view of the same kernel rides along
                if not roof.get("mfma_view"):
                    roof["mfma_view"] = rbp[dom]["mfma"]
                if not roof.get("hbm_view"):
                    roof["hbm_view"] = rbp[dom]["hbm"]
        return roof, phases

    if rank == 0 and not args.stub:
        result["roofline"], result["phases"] = roofline_of(net, precision)
        result["roofline_by_phase"] = result["roofline"].pop("by_phase", None)
        # host cost of a forward (Python + ctypes + the launches of ~16 kernels): the small inputs and the pairwise matrices are handed
        # over on the HOST, so nothing is read back from the device; each call is timed from entry to return on a drained stream (the
        # only blocking piece left inside is the 1.6 KB pageable copy of the pairwise matrices, which on a busy stream would wait for the
        # work queued before it - so the queue is kept empty instead of full).  What `--gpus 8` (eight such processes on one node) needs
        # is this figure well below the GPU's ms_per_step
        if not args.train:
            with torch.no_grad():
                hs = [scene[0]] + [t.cpu() for t in scene[1:]]
                for _ in range(3):
                    net(*hs)
                ts = []
                for _ in range(24):
                    sync()
                    t0 = time.perf_counter()
                    net(*hs)
                    ts.append(time.perf_counter() - t0)
                sync()
            ts.sort()
            result["host_ms_per_forward"] = {"value": ts[len(ts) // 2] * 1e3, "unit": "ms", "max": ts[-1] * 1e3,
                                             "what": "median wall time of one forward call, entry to return, stream drained before each call "
                                                     "(mode / record_len / mask / pairwise on the host: no device read-back); GPU time per "
                                                     "forward = ms_per_step"}
        side = not args.no_strict and world == 1
        if side:
            # a path that skips fully masked key tiles reports the dense figure too (same outputs,
            # tests/test_hip_fusion.py::test_skip_masked_is_exact)
            net.skip_masked = False
            k = max(2, args.steps // 4)
            result["dense_masked_tiles"] = {"value": k / timed(net, k, 1)[0], "unit": "scenes/s",
                                            "note": "every (ego, source, window) tile and every window of every agent computed, masked keys at -inf"}
            net.skip_masked = True
        if side and precision == "split":
            # the opt-in local-stage kernels of round 6: same results, fewer vector-memory wave loads
            for which, key in ((1, "patch_attention"), (2, "patch16_attention")):
                net.patch_attention = which
                pdt = timed(net, args.steps, args.warmup)[0]
                _, pph = roofline_of(net, precision)
                result[key] = {"value": args.steps / pdt, "unit": "scenes/s", "ms_per_step": pdt / args.steps * 1e3, "phases": pph,
                               "note": f"HeteroFusion.patch_attention = {which}: the local stages' attention on "
                                       + ("k_attention_patch (8 waves per window)" if which == 1 else "k_attention_patch16 (16 waves per window)")}
            net.patch_attention = 0
        del net
        torch.cuda.empty_cache()
        if side and precision != "f16":
            fast = make("f16")
            fdt = timed(fast, args.steps, args.warmup)[0]
            roof, ph = roofline_of(fast, "f16")
            result["fast_f16"] = {"value": args.steps / fdt, "unit": "scenes/s", "ms_per_step": fdt / args.steps * 1e3,
                                  "dtype": DTYPE["f16"], "tolerance": "1e-3 rel-max (north_star's figure), goldens g12 / g13",
                                  "roofline": roof, "phases": ph}
            del fast
            torch.cuda.empty_cache()
        if side and precision != "mixed" and c["C"] == 256:
            mixed = make("mixed")
            mdt = timed(mixed, args.steps, args.warmup)[0]
            roof, ph = roofline_of(mixed, "mixed")
            result["mixed_a16"] = {"value": args.steps / mdt, "unit": "scenes/s", "ms_per_step": mdt / args.steps * 1e3,
                                   "dtype": DTYPE["mixed"],
                                   "tolerance": "1e-4 rel-max on every parity case of tests/test_hip_fusion.py (goldens g12 / g13 "
                                                "included); not the headline because the f16 storage of Q / K' / V' / O is an "
                                                "input-dependent approximation of the reference's fp32 attention, the split mode is not",
                                   "roofline": roof, "phases": ph}
            del mixed
            torch.cuda.empty_cache()
        if side and precision != "f32":
            strict = make("f32")
            k = max(2, args.steps // 5)
            result["strict_f32"] = {"value": k / timed(strict, k, 1)[0], "unit": "scenes/s", "dtype": DTYPE["f32"]}
            del strict
        if side:
            # BASELINE configs[4] is the train loop: its fusion part on this GPU (HIP forward with dropout + HIP backward + AdamW,
            # hm-vit_amd/train.py) on the same scene, as a side figure
            torch.cuda.empty_cache()
            from hmvit_amd import train as T
            tnet = make("f32").train()
            opt = T.make_optimizer(tnet.parameters())
            target = torch.zeros(1, c["C"], c["H"], c["W"], device=dev)

            def train_once():
                opt.zero_grad()
                loss = (tnet(*scene) - target).pow(2).mean()
                loss.backward()
                opt.step()
            train_once()
            sync()
            t0 = time.perf_counter()
            k = 5
            for _ in range(k):
                train_once()
            sync()
            result["train_step"] = {"ms_per_step": (time.perf_counter() - t0) / k * 1e3, "unit": "ms",
                                    "what": "HeteroFusion forward (dropout 0.1) + backward + AdamW step on one scene of this workload, "
                                            "exact-f32 / split-f16 training kernels",
                                    "peak_memory_GiB": torch.cuda.max_memory_allocated(dev) / 2 ** 30}
            del tnet, opt, target
            torch.cuda.empty_cache()
        if side:
            result["other_configs"] = other_configs(args, dev, precision, hmvit_amd, S)
            result["encoders"], result["model_e2e"] = encoder_lines(dev, precision if precision != "mixed" else "split", hmvit_amd, S)
        if world == 1 and not args.no_cpu_baseline:
            result["cpu_baseline"] = cpu_baseline(c, args.num_iters, seed=1)
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
