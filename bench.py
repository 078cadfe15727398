#!/usr/bin/env python
"""Benchmark of the MI355X-native MeTRAbs per-crop hot path.

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]

A *step* is one pass of the hot path over one internal batch of synthetic input that is already
resident in HBM: BASELINE.json configs[1] = EfficientNetV2-S, 256 px crops, 64 crops per GPU,
num_aug=1.  Since round 4 a step of the weak-scaling configs is ONE CALL OF THE DROP-IN API --
Pose3dEstimator.estimate_poses_batched(frames on the device, host boxes, host cameras) with the
estimator's own HIP-graph cache -- on another of six frame sets every step (--step pipeline: the bare
replay of the captured internal batch that rounds 1-3 timed):

    uint8 1080p frames --(gamma decode + pyramid)--> (crop geometry) --> (perspective crop sampler)
      --> EfficientNetV2-S backbone [PyTorch-ROCm / MIOpen, random weights]
      --> (fused 1x1-projection MFMA + volumetric soft-argmax decode) --> (absolute reconstruction)
      --> (post-processing K7: mirror un-swap, back-rotation, 2D projection, TTA mean)
      --> poses3d [64, 17, 3], poses2d [64, 17, 2]                      (+ one all-gather if N > 1)

Parenthesised stages are the hand-written HIP kernels of libmetrabs_hip.so.  Metric: crops/sec,
whole job (all ranks).  Weak scaling: every rank processes its own 64 crops per step.

Prints ONE JSON line on rank 0: metric, value (crops/s), unit, higher_is_better, dtype, ms_per_step (one
timed step), steps, warmup and the workload.  A plain run does only that.  With --full the line also
carries ``roofline`` for the dominant hand-written kernel of the step, ``cpu_baseline`` for the CPU
restatement of the reference path (oracle/cpu_ref.py) timed on the host cores, and the other probes,
variants and parity checks (null in a plain run).  --dump-outputs DIR writes the last timed step's
result arrays as DIR/<name>.npy.
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # B/s spec (MI355X_MICROARCH.md); 6.29e12 measured float4 copy
HBM_COPY_MEASURED = 6.29e12
MFMA_F32_PEAK = 157.3e12   # FLOP/s, f32-in MFMA
MFMA_F16_PEAK = 2.5e15     # FLOP/s, dense f16 / bf16 MFMA (MI355X_MICROARCH.md)
MFMA_F64_PEAK = 78.6e12    # FLOP/s, f64 MFMA / vector

JOINT_NAMES = ['nose', 'leye', 'reye', 'lear', 'rear', 'lsho', 'rsho', 'lelb', 'relb', 'lwri', 'rwri',
               'lhip', 'rhip', 'lkne', 'rkne', 'lank', 'rank']
JOINT_EDGES = [(0, 1), (0, 2), (1, 3), (2, 4), (5, 6), (5, 7), (7, 9), (6, 8), (8, 10), (5, 11),
               (6, 12), (11, 12), (11, 13), (13, 15), (12, 14), (14, 16)]


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--config', type=int, default=1, choices=[1, 2, 3, 4],
                    help='BASELINE.json configs[N]: 1 = EffNetV2-S 256 px, 64 crops per GPU and step (weak '
                         'scaling, the metric\'s line); 2 = EffNetV2-L 384 px, 256 crops per step in internal '
                         'batches of 32 dealt round-robin to the ranks (strong scaling); 3 = MobileNetV3 '
                         '256 px, 8 frames x 8 boxes x num_aug 5 (with flips) = 320 crops per GPU and step '
                         '(weak; the sampler-bound case); 4 = EffNetV2-L 384 px under f16 autocast with a '
                         '122-joint head, 256 crops per step in internal batches of 32 (strong)')
    ap.add_argument('--total-crops', type=int, default=256, help='--config 2: crops per step, whole job')
    ap.add_argument('--backbone', default='effnetv2-s')
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--batch', type=int, default=64, help='crops per GPU per step')
    ap.add_argument('--num-aug', type=int, default=1)
    ap.add_argument('--frames', type=int, default=8, help='1080p frames per step per GPU')
    ap.add_argument('--joints', type=int, default=17)
    ap.add_argument('--depth', type=int, default=8,
                    help='depth bins of the volumetric heatmap (8 = every shipped config of the reference)')
    ap.add_argument('--no-depth72', action='store_true',
                    help="skip the extra timed run at the metric string's 72 depth bins")
    ap.add_argument('--no-fold-bn', action='store_true',
                    help='keep the backbone\'s batch norms as separate kernels (default: folded into '
                         'the convolutions, the usual inference-time transformation)')
    ap.add_argument('--no-fused-epilogue', action='store_true',
                    help='behind the folded convolutions, leave "+ bias" and the activation to PyTorch\'s '
                         'two elementwise kernels instead of the one in-place HIP pass (K10)')
    ap.add_argument('--precision', default='f32', choices=['f32', 'f16', 'bf16'],
                    help='backbone arithmetic: f32 = the reference CPU path; f16 = its autocast GPU path')
    ap.add_argument('--no-graph', action='store_true')
    ap.add_argument('--graph-gather', action='store_true',
                    help='N > 1, RCCL, weak scaling: capture the all-gather of the poses INSIDE the step\'s HIP graph '
                         '(one graph launch per step); falls back to the eager gather behind the replay -- and says '
                         'so in the line -- if the capture fails.  Off by default: it cannot be validated on a '
                         '1-GPU box')
    ap.add_argument('--force-collective', action='store_true',
                    help='--gpus 1: make a ONE-rank "nccl" (= RCCL) process group anyway and run the path\'s '
                         'all-gather of the poses in every step on device tensors (eager behind the replay, or '
                         'inside the graph with --graph-gather): RCCL load, communicator and the collective itself '
                         'exercised on a 1-GPU box; the line carries `multi_gpu` with backend "nccl"')
    ap.add_argument('--step', default='auto', choices=['auto', 'api', 'pipeline'],
                    help='what a timed step calls.  api (default for the weak-scaling configs 1 and 3): '
                         'Pose3dEstimator.estimate_poses_batched -- the drop-in surface itself, device-resident frames, '
                         'host boxes / cameras, the estimator\'s own HIP-graph cache; pipeline (configs 2 and 4, and '
                         '--graph-gather): a bare replay of the captured internal batch (GraphedCropPipeline)')
    ap.add_argument('--no-api-path', action='store_true',
                    help='skip the `api_path` probe (crops/s through Pose3dEstimator.estimate_poses_batched)')
    ap.add_argument('--full', action='store_true',
                    help='after the timed steps, run everything else the line can carry: per-kernel timing, '
                         'roofline probes (with the rocprofv3 PMC passes), parity probe, API-vs-pipeline check, '
                         'backbone / precision / depth variants and the CPU baseline.  Off by default: a plain run '
                         'sets up, warms up, times the steps and prints the contract line (those fields null)')
    ap.add_argument('--quick', action='store_true',
                    help='the contract line only, even with --full (what a plain run prints anyway)')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps, write what the last timed step returned (poses3d, poses2d, ...) '
                         'as DIR/<name>.npy in float32 / float64; the inputs are seeded, so two builds can be '
                         'compared output for output')
    ap.add_argument('--no-pmc', action='store_true',
                    help='do not run the two rocprofv3 --pmc passes that measure `roofline.traffic`')
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--no-decode-roofline', action='store_true')
    ap.add_argument('--cpu-seconds', type=float, default=20.0)
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be >= 1 and --warmup >= 0')
    if args.config in (2, 4):  # (explicit --backbone / --res / --batch still win when given)
        if args.backbone == 'effnetv2-s':
            args.backbone = 'effnetv2-l'
        if args.res == 256:
            args.res = 384
        if args.batch == 64:
            args.batch = 32
    if args.config == 4:  # multiperson_model.py:240-242 (autocast crop model), 122-joint head
        if args.precision == 'f32':
            args.precision = 'f16'
        if args.joints == 17:
            args.joints = 122
    if args.config == 3:  # multiperson_model.py:108-137 (the TTA table: rotations, scales, flips, gammas)
        if args.backbone == 'effnetv2-s':
            args.backbone = 'mobilenetv3'
        if args.num_aug == 1:
            args.num_aug = 5
        if args.batch == 64:
            args.batch = 64 * args.num_aug  # 8 frames x 8 boxes, every box sampled num_aug times
    args.strong = args.config in (2, 4)
    return args


def synth_inputs(pipe, frames, im_h, im_w, n_box, seed):
    """Seeded synthetic inputs written straight into the pipeline's static device buffers."""
    g = torch.Generator().manual_seed(seed)
    pipe.images.copy_(torch.randint(0, 256, (frames, 3, im_h, im_w), dtype=torch.uint8, generator=g))
    bw = 60 + 340 * torch.rand(n_box, generator=g)
    bh = 150 + 750 * torch.rand(n_box, generator=g)
    bx = torch.rand(n_box, generator=g) * (im_w - bw)
    by = torch.rand(n_box, generator=g) * (im_h - bh).clamp_min(1.0)
    pipe.boxes.copy_(torch.stack([bx, by, bw, bh], dim=1))
    f = max(im_h, im_w) / (np.tan(np.deg2rad(55.0) / 2) * 2)
    K = torch.tensor([[f, 0, im_w / 2], [0, f, im_h / 2], [0, 0, 1]], dtype=torch.float32)
    pipe.intrinsics.copy_(K.repeat(n_box, 1, 1))
    pipe.image_ids.copy_(((torch.arange(n_box) * frames) // n_box).int())   # frame-major: the order the API takes boxes in


def synthetic_crops(args, dev, im_h=1080, im_w=1920, seed=99, n_box=32):
    """Crops as the step's sampler produces them (synthetic frames, boxes and cameras of synth_inputs'
    kind, another seed): what the backbone's batch norms are calibrated on."""
    from metrabs_amd import kernels
    from metrabs_amd.multiperson.multiperson_model import tta_parameters
    g = torch.Generator().manual_seed(seed)
    frames = torch.randint(0, 256, (2, 3, im_h, im_w), dtype=torch.uint8, generator=g).to(dev)
    bw = 60 + 340 * torch.rand(n_box, generator=g)
    bh = 150 + 750 * torch.rand(n_box, generator=g)
    bx = torch.rand(n_box, generator=g) * (im_w - bw)
    by = torch.rand(n_box, generator=g) * (im_h - bh).clamp_min(1.0)
    boxes = torch.stack([bx, by, bw, bh], dim=1).to(dev)
    f = max(im_h, im_w) / (np.tan(np.deg2rad(55.0) / 2) * 2)
    K = torch.tensor([[f, 0, im_w / 2], [0, f, im_h / 2], [0, 0, 1]], dtype=torch.float32).repeat(n_box, 1, 1).to(dev)
    tta = {k: v.to(dev) for k, v in tta_parameters(args.num_aug).items()}
    with torch.inference_mode():
        _, _, wp = kernels.crop_geometry(
            boxes, K, torch.zeros(n_box, 12, device=dev), torch.tensor([0.0, -1.0, 0.0], device=dev).repeat(n_box, 1),
            (torch.arange(n_box) % 2).int().to(dev), tta['rotflipmat'], tta['scales'], tta['gammas'], args.res, 1)
        crops = kernels.warp_crops(kernels.build_pyramid(frames), wp, args.res, 1)
    return crops[torch.randperm(len(crops), generator=g)[:32].to(dev)].clone()


def build_model(args, dev):
    from metrabs_amd.backbones import build_backbone, calibrate_batchnorm, fold_batchnorm
    from metrabs_amd.config import MetrabsConfig
    from metrabs_amd.joint_info import JointInfo
    from metrabs_amd.models.metrabs import Metrabs
    from metrabs_amd.multiperson.multiperson_model import Pose3dEstimator
    # The backbone is PyTorch-ROCm (out of the hand-written scope); three backend choices were
    # measured for it (tools/experiments/*_probe.py).  (1) MIOpen's immediate mode falls back to its
    # naive direct convolution for the depthwise layers: those run on PyTorch's own depthwise
    # kernel instead (backbones.DepthwiseConv2d; 14.0 -> 13.1 ms).  (2) Inference-time batch norm is
    # folded into the preceding convolution (backbones.fold_batchnorm; 13.3 -> 11.8 ms; the same
    # function up to rounding, --no-fold-bn keeps the separate BN kernels), and "+ bias, activation"
    # behind each folded convolution is one in-place HIP pass (K10, csrc/bias_act.hip) instead of
    # PyTorch-ROCm's two elementwise kernels, with the blocks' skip connection and the squeeze-excite
    # mean riding on the same pass, and the depthwise 3x3 layers run with that epilogue as one HIP
    # pass over the plane (K11, csrc/depthwise.hip) (11.7 -> 8.8 ms; --no-fused-epilogue).  (3) MIOpen
    # benchmark mode: 2 minutes of search on a fresh box for the same step time, off
    # (MTR_BENCH_MIOPEN_FIND=1).
    if os.environ.get('MTR_BENCH_MIOPEN_FIND', '0') == '1':
        torch.backends.cudnn.benchmark = True
    if os.environ.get('MTR_BENCH_DETERMINISTIC') in ('0', '1'):   # (A/B of Metrabs.deterministic_backbone)
        Metrabs.deterministic_backbone = os.environ['MTR_BENCH_DETERMINISTIC'] == '1'
    torch.manual_seed(1234)
    cfg = MetrabsConfig(proc_side=args.res, depth=args.depth)
    names = JOINT_NAMES if args.joints == 17 else [f'j{i}' for i in range(args.joints)]
    edges = JOINT_EDGES if args.joints == 17 else [(i, i + 1) for i in range(args.joints - 1)]
    ji = JointInfo(names, edges)
    backbone = build_backbone(args.backbone)
    autocast = {'f32': None, 'f16': torch.float16, 'bf16': torch.bfloat16}[args.precision]
    model = Metrabs(backbone, ji, cfg, in_channels=backbone.out_channels, fused_head='auto',
                    autocast_dtype=autocast)
    model = model.to(dev)
    calibrate_batchnorm(model.backbone, args.res, dev, samples=synthetic_crops(args, dev))
    model = model.eval()
    reference_backbone = model.backbone  # the unfolded network: what the CPU baseline runs
    if not args.no_fold_bn:
        model.backbone = fold_batchnorm(model.backbone, fused_epilogue=not args.no_fused_epilogue)
    # (channels_last measured slower than NCHW on this MIOpen for both dtypes: 19.1 vs 14.0 ms in f32,
    #  15.0 vs 11.4 ms under f16 autocast -- tools/experiments/backbone_f16_probe.py)
    channels_last = os.environ.get('MTR_BENCH_CHANNELS_LAST') == '1'
    if channels_last:
        model = model.to(memory_format=torch.channels_last)
    skel = {'': dict(indices=list(range(args.joints)), names=names, edges=edges)}
    est = Pose3dEstimator(model, skel, None)
    object.__setattr__(est, 'reference_backbone', reference_backbone)  # (not a submodule of est)
    if autocast is not None:
        est.crop_dtype = autocast
    if channels_last:
        est.crop_channels_last = True
    return est, cfg


def kernels_mod():
    from metrabs_amd import kernels
    return kernels


def head_by_launch_size(est, args, n_crops):
    """The f32 fused head at the step's launch size and at one that fills the chip evenly.  At 64 crops
    of 8x8 maps a crop is 10 row tiles of 16 output channels: 640 tiles on 256 CUs = 3 + 3 + 3 + 1 per
    crop, i.e. at most 2.5 / 3 of the matrix pipes busy, plus ~5 us outside the K loop; the same kernel
    family at 1024 crops shows what the K loop itself reaches.  Random features, 20 launches per HIP-graph
    replay (graph_time)."""
    heads = est.crop_model.heatmap_heads
    C = est.crop_model.backbone.out_channels
    side = args.res // 32
    J, D = est.joint_info.n_joints, heads.config.depth
    g = torch.Generator(device='cuda').manual_seed(5)
    out = {}
    for B in sorted({n_crops, 1024}):
        feat = torch.randn(B, C, side, side, device='cuda', generator=g)
        us = graph_time([lambda: heads._forward_fused(feat)] * 20, 5) * 1e6
        flops = 2.0 * C * J * (1 + D) * side * side * B
        plan = kernels_mod().head_plan(B, C, side, side, J, D, torch.float32, False, True)
        out[str(B)] = dict(us_per_launch=round(us, 2), TFLOPs=round(flops / us / 1e6, 1),
                           frac_mfma=round(flops / (us * 1e-6) / MFMA_F32_PEAK, 3),
                           kernel=plan and plan['kernel'], workgroups=plan and plan['workgroups'])
    tiles = -(-J * (1 + D) // 16)
    out['note'] = (f'mtr_head_fused alone, f32 features; the step runs {n_crops} crops: {n_crops * tiles} row tiles '
                   f'of 16 output channels ({tiles} per crop) dealt to workgroups in whole tiles, on 256 CUs')
    return out


def depth72_variant(args, dev, im_h, im_w, n_box):
    """The metric string of BASELINE.json says "72 depth bins"; every shipped configuration of the
    reference uses depth = 8, which is what `value` is measured on.  This is the SAME step with a
    72-bin head (J*(1+72) = 1241 output channels) -- reported beside `value`, not instead of it.
    f32 features: the row-tile core of mtr_head_fused takes it (one joint = one atom of 5 row tiles);
    16-bit features: library GEMM + mtr_softargmax_decode."""
    import copy
    from metrabs_amd.pipeline import GraphedCropPipeline
    a72 = copy.copy(args)
    a72.depth = 72
    est72, _ = build_model(a72, dev)
    pipe = GraphedCropPipeline(est72, args.frames, im_h, im_w, n_box, num_aug=args.num_aug,
                               use_graph=not args.no_graph)
    synth_inputs(pipe, args.frames, im_h, im_w, n_box, seed=100)
    pipe.capture()
    for _ in range(3):
        pipe.run()
    torch.cuda.synchronize()
    n = max(5, args.steps // 2)
    t0 = time.perf_counter()
    for _ in range(n):
        pipe.run()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / n * 1e3
    assert torch.isfinite(pipe.poses).all()
    heads = est72.crop_model.heatmap_heads
    C = est72.crop_model.backbone.out_channels
    hw = args.res // 32
    fused = heads.last_path == 'fused'
    return dict(crops_per_s_per_gpu=n_box * args.num_aug / ms * 1e3, ms_per_step=ms, steps=n,
                head=('mtr_head_fused (row-tile core: a joint\'s 72 depth slices + 8 rows of 2D heatmaps '
                      'are one 5-tile atom, 17 atoms)' if fused else
                      '1x1 conv (library GEMM) + mtr_softargmax_decode, D=72'),
                head_chosen_by=f'MetrabsHeads(fused={heads.fused!r}): kernels.head_auto_choice, a static rule on '
                               f'(dtype, layout, C, H, W, J, D) -- no timing, no batch size',
                note='same step as `value` with a 72-bin head; `value` itself uses depth=8 '
                     '(every shipped configuration of the reference)')


def backbone_variant(args, dev, im_h, im_w, n_box, fold_bn, fused_epilogue, note):
    """`value` runs the backbone's inference copy with batch norm folded into the convolutions and
    the K10 / K11 epilogue kernels (the same function up to rounding).  For transparency: the SAME
    step with less of that, reported beside `value`."""
    import copy
    from metrabs_amd.pipeline import GraphedCropPipeline
    a = copy.copy(args)
    a.no_fold_bn = not fold_bn
    a.no_fused_epilogue = not fused_epilogue
    est, _ = build_model(a, dev)
    pipe = GraphedCropPipeline(est, args.frames, im_h, im_w, n_box, num_aug=args.num_aug,
                               use_graph=not args.no_graph)
    synth_inputs(pipe, args.frames, im_h, im_w, n_box, seed=100)
    pipe.capture()
    for _ in range(3):
        pipe.run()
    torch.cuda.synchronize()
    n = max(5, args.steps // 2)
    t0 = time.perf_counter()
    for _ in range(n):
        pipe.run()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / n * 1e3
    assert torch.isfinite(pipe.poses).all()
    return dict(crops_per_s_per_gpu=n_box * args.num_aug / ms * 1e3, ms_per_step=ms, steps=n, note=note)


def autocast_variant(args, dev, im_h, im_w, n_box, precision='f16'):
    """The reference's own GPU arithmetic: it runs the crop model under torch.autocast(float16) on a GPU
    (multiperson_model.py:241).  The SAME step with the backbone under f16 autocast, 16-bit crops from the
    sampler and the f16-MFMA fused head -- reported beside `value` (which keeps the f32 arithmetic of the
    reference's CPU path, the parity target)."""
    import copy
    from metrabs_amd.pipeline import GraphedCropPipeline
    a = copy.copy(args)
    a.precision = precision
    est, _ = build_model(a, dev)
    pipe = GraphedCropPipeline(est, args.frames, im_h, im_w, n_box, num_aug=args.num_aug,
                               use_graph=not args.no_graph)
    synth_inputs(pipe, args.frames, im_h, im_w, n_box, seed=100)
    pipe.capture()
    for _ in range(3):
        pipe.run()
    torch.cuda.synchronize()
    n = max(5, args.steps // 2)
    t0 = time.perf_counter()
    for _ in range(n):
        pipe.run()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / n * 1e3
    assert torch.isfinite(pipe.poses).all()
    heads = est.crop_model.heatmap_heads
    J, C = est.joint_info.n_joints, est.crop_model.backbone.out_channels
    return dict(crops_per_s_per_gpu=n_box * args.num_aug / ms * 1e3, ms_per_step=ms, steps=n, dtype=precision,
                head=head_kernel_name((args.res // 32) ** 2, n_box * args.num_aug, J, heads.config.depth, precision, C)
                if heads.last_path == 'fused' else 'library 1x1 conv + mtr_softargmax_decode',
                note='same step as `value` with the crop model under torch.autocast(float16) -- the reference\'s '
                     'GPU arithmetic (multiperson_model.py:241); 16-bit crops, f16-MFMA fused head')


def head_kernel_name(hw, n_crops, J, D, precision='f32', C=1280):
    """Which kernel mtr_head_fused_ws takes for the launch -- asked of the library itself
    (mtr_head_plan, host-only), not mirrored here."""
    from metrabs_amd import kernels
    side = int(round(hw ** 0.5))
    dt = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}[precision]
    plan = kernels.head_plan(n_crops, C, side, hw // side, J, D, dt)
    if plan is None:
        return 'library 1x1 conv (rocBLAS / MIOpen) + decode_nchw_kernel'
    name = plan['kernel']
    if plan['split_column_blocks']:
        name += f' (+ head_rt_merge_kernel: {plan["split_column_blocks"]} column blocks over workgroups)'
    return name


def graph_time(calls, replays):
    """Average duration of one call: the list of zero-argument `calls` is captured ONCE into a HIP
    graph (so that no Python / ctypes / allocator time sits between the launches) and the graph is
    replayed `replays` times between two HIP events on the capture stream."""
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st), torch.inference_mode():
        for c in calls:  # lazy initialisation outside the capture
            c()
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st, capture_error_mode='thread_local'):  # (see metrabs_amd/pipeline.py)
            for c in calls:
                c()
        g.replay()
        st.synchronize()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record(st)
        for _ in range(replays):
            g.replay()
        stop.record(st)
        st.synchronize()
    torch.cuda.current_stream().wait_stream(st)
    return start.elapsed_time(stop) * 1e-3 / (replays * len(calls))


def time_stage(fn, iters, warm=3):
    """One stage on its own, cache-hot inputs: `iters` launches inside one graph, 3 replays."""
    return graph_time([fn] * max(1, iters), 3)


def stage_breakdown(pipe, est, args, iters):
    """Average duration of every stage of the step, measured with HIP events on the stream the
    kernels are launched on (torch's current stream)."""
    from metrabs_amd import kernels
    res, aa = args.res, 1
    tta = pipe.tta
    model = est.crop_model
    st = {}
    with torch.inference_mode():
        st['pyramid'] = time_stage(lambda: kernels.build_pyramid(pipe.images), iters)
        pyr = kernels.build_pyramid(pipe.images)
        geo = lambda: kernels.crop_geometry(
            pipe.boxes, pipe.intrinsics, pipe.distortion12, pipe.camspace_up, pipe.image_ids,
            tta['rotflipmat'], tta['scales'], tta['gammas'], res, aa)
        st['geometry'] = time_stage(geo, iters)
        new_k, rot, wp = geo()
        warp = lambda: kernels.warp_crops(pyr, wp, res, aa, out_dtype=est.crop_dtype,
                                          channels_last=est.crop_channels_last)
        st['warp'] = time_stage(warp, iters)
        crops = warp()

        def backbone():
            if model.autocast_dtype is not None:
                with torch.autocast('cuda', dtype=model.autocast_dtype):
                    return model.backbone(crops)
            return model.backbone(crops)
        st['backbone'] = time_stage(backbone, max(3, iters // 3))
        feats = backbone()
        heads = model.heatmap_heads
        st['head_fused'] = time_stage(lambda: heads(feats), iters)
        c2d, c3d = heads(feats)
        kflat = new_k.reshape(-1, 3, 3)
        ws = kernels.reconstruct_workspace(c2d.shape[0], c2d.shape[1], c2d.device)
        st['reconstruct'] = time_stage(
            lambda: kernels.reconstruct_absolute(c2d, c3d, kflat, model.config, workspace=ws), iters)
        poses_flat = kernels.reconstruct_absolute(c2d, c3d, kflat, model.config, workspace=ws)
        st['postprocess'] = time_stage(lambda: kernels.postprocess_poses(
            poses_flat, rot, tta['should_flip_u8'], tta['mirror_i32'], pipe.intrinsics, pipe.distortion12,
            pipe.inv_extrinsics, None, None, True), iters)
    return st, dict(wp=wp, crops=crops, feats=feats, c2d=c2d, c3d=c3d, kflat=kflat)


ROTATE_BYTES = 640 << 20   # > 2x the 256 MiB Infinity Cache: what a kernel reads is not still on die


def time_rotating(make_call, n_sets, iters, warm=None):
    """Average launch duration of make_call(i): every launch of the captured graph works on another
    input set, n_sets of them spanning more than ROTATE_BYTES (nothing it reads is still on die)."""
    calls = [(lambda i=i: make_call(i)) for i in range(n_sets)]
    return graph_time(calls, max(2, -(-iters // n_sets)))


def rotating_sampler_times(pipe, est, args, wp, iters):
    """Pyramid and sampler on frames that are NOT the ones the previous launch touched: the step
    itself re-reads the same 50 MB of frames + 14 MB of pyramid every iteration, well inside the
    Infinity Cache, so its stage times are cache-assisted; these are the HBM-true ones."""
    from metrabs_amd import kernels
    frame_bytes = pipe.images.numel()
    n_sets = max(2, -(-ROTATE_BYTES // (frame_bytes + frame_bytes // 3)))
    g = torch.Generator(device=pipe.images.device).manual_seed(17)
    with torch.inference_mode():
        frames = [torch.randint(0, 256, pipe.images.shape, dtype=torch.uint8, device=pipe.images.device,
                                generator=g) for _ in range(n_sets)]
        t_pyr = time_rotating(lambda i: kernels.build_pyramid(frames[i]), n_sets, iters)
        pyrs = [kernels.build_pyramid(f) for f in frames]
        t_warp = time_rotating(lambda i: kernels.warp_crops(
            pyrs[i], wp, args.res, 1, out_dtype=est.crop_dtype, channels_last=est.crop_channels_last),
            n_sets, iters)
        # the same frames with interleaved channels ([N,H,W,3] memory, channels_last): what a decoder hands over;
        # sampled in place by mtr_build_pyramid_u8_hwc / mtr_warp_crops_u8_hwc (two gathers per sample, not six)
        del pyrs
        frames = [f.contiguous(memory_format=torch.channels_last) for f in frames]
        t_pyr_il = time_rotating(lambda i: kernels.build_pyramid(frames[i]), n_sets, iters)
        pyrs = [kernels.build_pyramid(f) for f in frames]
        assert all(p.hwc for p in pyrs)
        t_warp_il = time_rotating(lambda i: kernels.warp_crops(
            pyrs[i], wp, args.res, 1, out_dtype=est.crop_dtype, channels_last=est.crop_channels_last),
            n_sets, iters)
    del frames, pyrs
    torch.cuda.empty_cache()
    return dict(pyramid=t_pyr, warp=t_warp, n_sets=n_sets, pyramid_interleaved=t_pyr_il, warp_interleaved=t_warp_il)


def detector_pre_probe(pipe, iters):
    """K9 (row f.3 of SURVEY section 8): PersonDetector's pre-processing of the step's own frames --
    gamma-correct antialiased resize to 416 px + pad -- which `detect_poses` runs in front of the path
    `value` times (the detector network between them is third party).  Frames rotated over more than
    the Infinity Cache; algorithmic bytes = the uint8 frames once + the f32 network input once."""
    from metrabs_amd import kernels
    n, _, h, w = pipe.images.shape
    geom = kernels.detector_geometry(h, w)
    n_sets = max(2, -(-ROTATE_BYTES // pipe.images.numel()))
    g = torch.Generator(device=pipe.images.device).manual_seed(23)
    with torch.inference_mode():
        frames = [torch.randint(0, 256, pipe.images.shape, dtype=torch.uint8, device=pipe.images.device, generator=g)
                  for _ in range(n_sets)]
        out = torch.empty(n, 3, geom.out_h, geom.out_w, device=pipe.images.device)
        t = time_rotating(lambda i: kernels.detector_preprocess(frames[i], geom=geom, out=out), n_sets, iters)
    nbytes = pipe.images.numel() + out.numel() * 4
    del frames
    torch.cuda.empty_cache()
    return dict(kernel='detector_stream_kernel / detector_pre_kernel (by launch size)', launches=1,
                us=round(t * 1e6, 2), GBps=round(nbytes / t / 1e9, 1), frac_hbm=round(nbytes / t / HBM_PEAK, 4),
                frames=list(pipe.images.shape),
                note='instruction-issue-bound (one LUT lookup + fma per tap, 108 M taps per 8 x 1080p): '
                     'DESIGN.md section 3, K9')


def backbone_epilogue_kernels(est, crops, iters):
    """K10 (bias_act_kernel) and K11 (depthwise3x3_kernel) sit inside the PyTorch backbone of `value`
    (backbones.fold_batchnorm(fused_epilogue=True)).  One eager forward records every launch
    (shapes, dtype, options); every distinct launch is then replayed on rotating buffers spanning
    more than the Infinity Cache and timed with HIP events on the launch stream.  -> per kernel:
    launches per step, their summed duration and summed ALGORITHMIC bytes (each activation read
    once and written once, the skip connection read once; weights / bias / means once)."""
    from metrabs_amd import kernels
    model = est.crop_model
    calls = []
    orig = (kernels.bias_act_, kernels.bias_act_rowmean_, kernels.depthwise3x3_bias_act)

    def rec_bias(y, bias, act, residual=None):
        calls.append(('bias_act', tuple(y.shape), y.dtype, act, residual is not None, False))
        return orig[0](y, bias, act, residual)

    def rec_rowmean(y, bias, act):
        calls.append(('bias_act', tuple(y.shape), y.dtype, act, False, True))
        return orig[1](y, bias, act)

    def rec_dw(x, weight, bias, act, stride, pad, want_mean=False):
        pad = (int(pad),) * 4 if isinstance(pad, int) else tuple(int(p) for p in pad)  # (l, r, t, b)
        calls.append(('depthwise', tuple(x.shape), x.dtype, act, int(stride), pad, bool(want_mean)))
        return orig[2](x, weight, bias, act, stride, pad, want_mean)

    kernels.bias_act_, kernels.bias_act_rowmean_, kernels.depthwise3x3_bias_act = rec_bias, rec_rowmean, rec_dw
    try:
        with torch.inference_mode():
            if model.autocast_dtype is not None:
                with torch.autocast('cuda', dtype=model.autocast_dtype):
                    model.backbone(crops)
            else:
                model.backbone(crops)
    finally:
        kernels.bias_act_, kernels.bias_act_rowmean_, kernels.depthwise3x3_bias_act = orig
    if not calls:
        return {}
    counts = {}
    for c in calls:
        counts[c] = counts.get(c, 0) + 1
    out = {}
    dev = crops.device
    g = torch.Generator(device=dev).manual_seed(23)
    for sig, n in counts.items():
        kind, shape, dtype = sig[0], sig[1], sig[2]
        es = torch.empty((), dtype=dtype).element_size()
        numel = int(np.prod(shape))
        B, C = shape[0], shape[1]
        if kind == 'bias_act':
            _, _, _, act, has_res, want_mean = sig
            nbytes = numel * es * (3 if has_res else 2) + C * 4 + (B * C * 4 if want_mean else 0)
            n_sets = max(2, min(64, -(-ROTATE_BYTES // (numel * es * (2 if has_res else 1)))))
            ys = [torch.randn(shape, device=dev, generator=g).to(dtype) for _ in range(n_sets)]
            rs = [torch.randn(shape, device=dev, generator=g).to(dtype) for _ in range(n_sets)] if has_res else None
            bias = torch.randn(C, device=dev, generator=g) * 0.1
            if want_mean:
                call = lambda i: orig[1](ys[i], bias, act)
            else:
                call = lambda i: orig[0](ys[i], bias, act, rs[i] if has_res else None)
            name = 'bias_act_kernel'
        else:
            _, _, _, act, stride, pad, want_mean = sig
            H, W = shape[2], shape[3]
            OH, OW = (H + pad[2] + pad[3] - 3) // stride + 1, (W + pad[0] + pad[1] - 3) // stride + 1
            nbytes = numel * es + B * C * OH * OW * es + C * 10 * 4 + (B * C * 4 if want_mean else 0)
            n_sets = max(2, min(64, -(-ROTATE_BYTES // (numel * es))))
            xs = [torch.randn(shape, device=dev, generator=g).to(dtype) for _ in range(n_sets)]
            wgt = torch.randn(C, 3, 3, device=dev, generator=g) * 0.3
            bias = torch.randn(C, device=dev, generator=g) * 0.1
            call = lambda i: orig[2](xs[i], wgt, bias, act, stride, pad, want_mean)
            name = 'depthwise3x3_kernel'
        with torch.inference_mode():
            t = time_rotating(call, n_sets, max(iters, 2 * n_sets))
            # ... and on ONE buffer set: what the launch costs inside the step, where the activation
            # was written by the convolution in front a moment ago (hip_share_of_step uses this one)
            t_hot = graph_time([lambda: call(0)] * 8, 3)
        e = out.setdefault(name, dict(launches_per_step=0, seconds_per_step=0.0, bytes_per_step=0, slowest=None,
                                      hot_seconds_per_step=0.0))
        e['launches_per_step'] += n
        e['seconds_per_step'] += n * t
        e['hot_seconds_per_step'] += n * t_hot
        e['bytes_per_step'] += n * nbytes
        frac = nbytes / t / HBM_PEAK
        if e['slowest'] is None or frac < e['slowest']['frac_hbm']:
            e['slowest'] = dict(shape=list(shape), dtype=str(dtype).replace('torch.', ''), us=round(t * 1e6, 2),
                                frac_hbm=round(frac, 4), options=[str(x) for x in sig[3:]])
        if os.environ.get('MTR_BENCH_LAUNCH_TABLE'):  # developer aid: one line per distinct launch
            with open(os.environ['MTR_BENCH_LAUNCH_TABLE'], 'a') as f:
                f.write(json.dumps(dict(kernel=name, shape=list(shape), options=[str(x) for x in sig[2:]],
                                        launches=n, us=round(t * 1e6, 2), MB=round(nbytes / 1e6, 2),
                                        frac_hbm=round(frac, 4))) + '\n')
        del call
        torch.cuda.empty_cache()
    return out



def source_footprint_bytes(wp, res, im_h, im_w):
    """Clipped axis-aligned bounding box (in texels of the chosen pyramid level) of each warped crop
    quad -- SURVEY.md 8(d) S_src -- times 3 planes x 4 B."""
    wp = wp.detach().cpu().double()
    total = 0.0
    corners = torch.tensor([[0.0, 0.0, 1.0], [res - 1.0, 0.0, 1.0], [0.0, res - 1.0, 1.0],
                            [res - 1.0, res - 1.0, 1.0]], dtype=torch.float64)
    for row in wp:
        hinv, kl, lvl = row[0:9].reshape(3, 3), row[9:18].reshape(3, 3), int(row[31])
        rays = corners @ hinv.T
        n = rays[:, :2] / rays[:, 2:]
        q = torch.cat([n, torch.ones(4, 1, dtype=torch.float64)], dim=1) @ kl.T
        w, h = (im_w >> lvl), (im_h >> lvl)
        x0, x1 = q[:, 0].min().clamp(0, w - 1), q[:, 0].max().clamp(0, w - 1)
        y0, y1 = q[:, 1].min().clamp(0, h - 1), q[:, 1].max().clamp(0, h - 1)
        # level 0 is sampled from the uint8 frame (1 B / texel); levels 1-2 are f32
        total += float((x1 - x0 + 1) * (y1 - y0 + 1)) * 3 * (1 if lvl == 0 else 4)
    return total


def decode_roofline(iters=20, nhwc=False, shape=(32768, 17, 8, 8)):
    """K2-K4 standalone on a batch beyond the 256 MiB Infinity Cache: J=17, 8x8, D=8, B=32768
    (1.28 GB of fp32 logits).  nhwc: the same logits in the TF twin's layout
    ('b h w (d j)', metrabs_tf/models/metrabs.py:100-101; torch channels_last) through the NHWC kernels of csrc/decode.hip."""
    from metrabs_amd import kernels
    from metrabs_amd.config import MetrabsConfig
    B, J, D, side = shape
    g = torch.Generator(device='cuda').manual_seed(3)
    logits = torch.randn(B, J * (1 + D), side, side, device='cuda', generator=g)
    if nhwc:
        logits = logits.contiguous(memory_format=torch.channels_last)
    cfg = MetrabsConfig(depth=D, proc_side=side * 32)
    out = (torch.empty(B, J, 2, device='cuda'), torch.empty(B, J, 3, device='cuda'))
    t = time_stage(lambda: kernels.softargmax_decode(logits, J, cfg, out=out), iters)
    bytes_per_crop = J * (1 + D) * side * side * 4 + 20 * J
    achieved = B * bytes_per_crop / t
    del logits
    torch.cuda.empty_cache()
    return dict(kernel='decode_nhwc_staged_kernel<float> (LDS ring fed by global_load_lds; >= 256 crops of <= 1,024 channels), else decode_nhwc_kernel<float>'
                if nhwc else 'decode_nchw_kernel<float,4,16>', bound='hbm',
                achieved=achieved / 1e9, peak=HBM_PEAK / 1e9, unit='GB/s', frac=achieved / HBM_PEAK,
                frac_of_measured_copy=achieved / HBM_COPY_MEASURED, avg_launch_us=t * 1e6,
                crops=B, bytes_per_crop=bytes_per_crop, traffic=None)


def cpu_baseline(est, pipe, args, cfg, seconds):
    """The CPU restatement of the reference path (oracle/cpu_ref.py, pinned bit-for-bit to the
    reference on the golden vectors) on this box's host cores, same synthetic workload, bounded
    sample."""
    from oracle import cpu_ref
    ocfg = cpu_ref.HeadConfig(proc_side=cfg.proc_side)
    model = est.crop_model
    # the network as the reference runs it (batch norms as their own ops, torch kernels only), not
    # the folded inference copy the GPU step uses
    backbone = copy.deepcopy(getattr(est, 'reference_backbone', model.backbone)).to('cpu', torch.float32).eval()
    w = model.heatmap_heads.conv_final.weight.detach().cpu().float()
    b = model.heatmap_heads.conv_final.bias.detach().cpu().float()
    J = model.joint_info.n_joints
    mirror = model.joint_info.mirror_mapping

    def crop_model(inp):
        crops, K = inp
        return cpu_ref.crop_model_from_features(backbone(crops), w, b, K, J, ocfg)

    images = pipe.images.cpu()
    boxes_all = torch.cat([pipe.boxes.cpu(), torch.ones(len(pipe.boxes), 1)], dim=1)
    ids = pipe.image_ids.cpu().long()
    K = pipe.intrinsics[:1].cpu()

    def run(n_box):
        per_image = [boxes_all[:n_box][ids[:n_box] == i] for i in range(len(images))]
        with torch.inference_mode():
            return cpu_ref.estimate_poses_batched(
                crop_model, mirror, J, args.res, images, per_image, K, torch.zeros(1, 5),
                torch.eye(4)[None], torch.tensor([0.0, -1.0, 0.0]), 55, args.batch * args.num_aug,
                1, args.num_aug, True)

    # Thread count: torch's default (all hardware threads) is NOT the fastest setting of this path
    # on a many-core host (per-crop Python loops + small ops oversubscribe), and the reference
    # itself pins OMP_NUM_THREADS=1 (metrabs_pytorch/init.py:3).  The SAME batch -- all of the
    # step's crops on all of its frames -- is timed at each thread count after one warm-up call on a
    # small batch at that count; `value` is the best of them, `one_thread` the reference's own
    # setting, and crops_per_s_by_threads holds every one (same workload, so they are comparable).
    all_threads = torch.get_num_threads()
    host_cpus = os.cpu_count() or all_threads   # hardware threads of the host (torch's default count on the GPU box)
    n_box = args.batch // args.num_aug
    crops = n_box * args.num_aug
    by_threads, secs, sample_boxes, gave_up = {}, {}, {}, {}
    per_count = max(seconds, 5.0)
    budget_end = time.time() + per_count * 3.0

    def bounded(fn, limit):
        """fn() under a wall-clock limit (SIGALRM raises between the oracle's Python-level steps; main thread) -> done?"""
        import signal

        class _Late(Exception):
            pass

        def on_alarm(signum, frame):
            raise _Late()
        try:
            old = signal.signal(signal.SIGALRM, on_alarm)
        except ValueError:  # (not the main thread: no limit)
            fn()
            return True
        signal.alarm(max(1, int(limit)))
        try:
            fn()
            return True
        except _Late:
            return False
        finally:
            signal.alarm(0)
            signal.signal(signal.SIGALRM, old)
    try:
        # 8, the reference's own 1, EVERY hardware thread (the all-cores run was never tried; it is
        # torch's default on the GPU box), torch's default where that differs, 32; `cores` = the count that produced
        # `value`.  Every call runs under a wall-clock limit: all 256 threads of the GPU box's host need ~100 s for TWO
        # boxes (0.02 crops/s; 0.24 on the whole batch, 267 s -- round 6: torch's small ops oversubscribe), which a
        # bench line cannot afford; a count that does not finish says so in `did_not_finish`.  A count whose warm-up
        # says the whole batch would not fit its share of the budget is timed on as many boxes as fit, at least 2
        # (`boxes_timed_by_threads`)
        for t in dict.fromkeys((8, 1, host_cpus, all_threads, 32)):
            if t > host_cpus or (len(by_threads) >= 3 and time.time() > budget_end):
                continue
            torch.set_num_threads(t)
            w0 = time.time()
            # warm-up at this setting (thread pool, oneDNN primitives, allocator)
            if not bounded(lambda: run(min(2, n_box)), per_count):
                gave_up[t] = f'the warm-up call on {min(2, n_box)} boxes did not finish within {per_count:.0f} s'
                continue
            warm = time.time() - w0
            fit = int(n_box * per_count / max(warm / min(2, n_box) * n_box, 1e-9))
            n_t = n_box if fit >= n_box else max(2, min(n_box, fit))
            t0 = time.time()
            if not bounded(lambda: run(n_t), 2 * per_count):
                gave_up[t] = f'{n_t} boxes did not finish within {2 * per_count:.0f} s (warm-up on 2 boxes: {warm:.1f} s)'
                continue
            secs[t] = time.time() - t0
            sample_boxes[t] = n_t
            by_threads[t] = n_t * args.num_aug / secs[t]
    finally:
        torch.set_num_threads(all_threads)
    best = max(by_threads, key=by_threads.get)
    return dict(value=by_threads[best], unit='crops/s', cores=best, kind='port',
                sample=f'1 x {sample_boxes[best] * args.num_aug} crops ({args.frames} 1080p frames): the same step as the GPU '
                       f'(gamma decode + pyramid + sampler + {args.backbone} fp32 + head + '
                       f'reconstruction), oracle/cpu_ref.py on torch CPU, timed once per thread count after '
                       f'a warm-up call at 1 / 8 / 32 / {all_threads} (torch\'s default) / {host_cpus} (every hardware '
                       f'thread) threads; value = the fastest count ({best} of the host\'s {host_cpus})',
                seconds_per_batch=secs[best], host_threads=host_cpus, torch_default_threads=all_threads,
                boxes_timed_by_threads={str(k): v for k, v in sorted(sample_boxes.items())},
                all_cores=dict(value=by_threads.get(host_cpus), unit='crops/s', cores=host_cpus,
                               did_not_finish=gave_up.get(host_cpus)),
                did_not_finish={str(k): v for k, v in sorted(gave_up.items())},
                crops_per_s_by_threads={str(k): round(v, 2) for k, v in sorted(by_threads.items())},
                one_thread=dict(value=by_threads.get(1), unit='crops/s', cores=1,
                                sample='the same batch under torch.set_num_threads(1) (the reference pins '
                                       'OMP_NUM_THREADS=1, metrabs_pytorch/init.py:3)'),
                reference_in_build_container={
                    'crops_per_s_by_threads': {'1': 7.78, '8': 31.2},
                    'port_on_the_same_host': {'1': 8.60, '8': 35.3},
                    'max_abs_pose_difference_mm': 0.0,
                    'note': 'the REAL reference (metrabs_pytorch Pose3dEstimator + Metrabs + efficientnet_v2_s run '
                            'in place by oracle/time_reference.py) beside this port on the build container\'s 8 '
                            'vCPUs, 8 crops of one 1080p frame; /root/reference does not exist on the GPU box, '
                            'hence kind = "port" here'})


def _parity_numbers(ours, ref, truth):
    from oracle import cpu_ref
    return dict(mpjpe_mm=cpu_ref.mpjpe(ours, ref), max_abs_mm=float((ours - ref).abs().max()),
                ours_vs_fp64_mpjpe_mm=cpu_ref.mpjpe(ours, truth),
                ref_vs_fp64_mpjpe_mm=cpu_ref.mpjpe(ref, truth),
                ours_vs_fp64_max_mm=float((ours.double() - truth).abs().max()),
                ref_vs_fp64_max_mm=float((ref.double() - truth).abs().max()),
                median_depth_mm=float(truth[..., 2].median()))


def parity_probe(est, extras, cfg, args):
    """MPJPE (mm) of the HIP head + reconstruction vs the oracle on IDENTICAL backbone features
    (the north-star parity definition), in three regimes at the bench's own shape
    (tests/test_gpu_parity_gates.py gates the same regimes at every BASELINE config shape):

    consistent_low / consistent_peaked -- features + a default-initialised conv_final whose logits
        describe a plausible pose 2.5 - 4.5 m from the camera (oracle/cases.consistent_head_case),
        logits <= 5 resp. ~25: the 1e-3 mm bound is met;
    bench_batch_random_network -- the features the bench's random-weight backbone just produced:
        nearly uniform heatmaps, every joint decodes to the crop centre, the reference-point depth
        is the ratio of two vanishing spreads (median depth ~0 mm) and the oracle's own fp32 result
        is ~1e-2 mm from an fp64 evaluation of the same formulas; *_vs_fp64 shows whose noise it is."""
    from oracle import cases, cpu_ref
    from metrabs_amd import kernels
    model = est.crop_model
    ocfg = cpu_ref.HeadConfig(proc_side=cfg.proc_side, depth=cfg.depth)
    J = model.joint_info.n_joints
    out = {'definition': 'poses3d (mm) from identical features: ours = mtr_head_fused + '
                         'mtr_reconstruct_absolute through the C-ABI; ref = oracle/cpu_ref.py (fp32 CPU '
                         'restatement of metrabs_pytorch, pinned to it); fp64 = the same formulas in float64'}
    try:  # the reference against itself, run to run (oracle/gen_golden.py jitter, build container)
        jitter = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'parity_reference_jitter.json')))
    except (OSError, ValueError):
        jitter = {}
    feats = extras['feats']
    B, C, H, W = feats.shape
    # the bench's shape is one of the parity-gate shapes (configs[1] by default): compare with the
    # STORED output of the reference itself (tests/golden/parity_*.npz, minted in the build container
    # by running metrabs_pytorch's MetrabsHeads.forward + reconstruct_absolute) instead of the port
    # evaluated on this box's CPU
    gate = next((n for n, sh in cases.PARITY_GATE_SHAPES.items()
                 if sh == (B, C, J, H, cfg.proc_side, cfg.depth, feats.dtype) and H == W), None)
    for regime, amp in (('consistent_low', 4.0), ('consistent_peaked', 25.0)):
        stored = None
        if gate is not None:
            path = os.path.join(ROOT, 'tests', 'golden', cases.parity_gate_slug(gate, regime) + '.npz')
            if os.path.exists(path):
                stored = np.load(path)
        if stored is not None:
            feat, w, b, K = cases.parity_gate_inputs(gate, regime)
        else:
            feat, w, b, K = cases.consistent_head_case(B, C, J, H, cfg.proc_side, cfg.depth, amp, seed=4242)
            feat = feat.to(feats.dtype)
        with torch.inference_mode():
            if stored is not None:
                ref, truth = torch.from_numpy(stored['poses3d']), torch.from_numpy(stored['poses3d_fp64'])
            else:
                wk = cases.head_weights_as_consumed(w, feats.dtype)
                ref = cpu_ref.crop_model_from_features(feat.float(), wk, b, K, J, ocfg)
                truth = cpu_ref.crop_model_from_features_fp64(feat.float(), wk, b, K, J, ocfg)
            packed = kernels.head_pack_weights(w.cuda(), b.cuda(), J, cfg.depth, feats.dtype)
            c2d, c3d = kernels.head_fused(feat.cuda(), packed, C, J, model.config)
            ours = kernels.reconstruct_absolute(c2d, c3d, K.cuda(), model.config).cpu()
        out[regime] = _parity_numbers(ours, ref, truth)
        out[regime]['logits_peak'] = amp
        if gate is not None and cases.parity_gate_slug(gate, regime) in jitter:
            jr = jitter[cases.parity_gate_slug(gate, regime)]
            out[regime]['reference_run_to_run_max_mm'] = jr['run_to_run_max_mm']
            out[regime]['reference_run_to_run_mpjpe_mm'] = jr['run_to_run_mpjpe_mm']
        out[regime]['ref_is'] = ('stored output of the reference itself (tests/golden/' +
                                 cases.parity_gate_slug(gate, regime) + '.npz)') if stored is not None else \
            'oracle/cpu_ref.py evaluated on this box\'s CPU'
    feats = feats.float().cpu()
    w = model.heatmap_heads.conv_final.weight.detach().cpu().float()
    b = model.heatmap_heads.conv_final.bias.detach().cpu().float()
    with torch.inference_mode():
        wk = cases.head_weights_as_consumed(w.reshape(w.shape[0], -1), extras['feats'].dtype)
        ref = cpu_ref.crop_model_from_features(feats, wk, b, extras['kflat'].cpu(), J, ocfg)
        truth = cpu_ref.crop_model_from_features_fp64(feats, wk, b, extras['kflat'].cpu(), J, ocfg)
        ours = kernels.reconstruct_absolute(extras['c2d'], extras['c3d'], extras['kflat'],
                                            model.config).cpu()
        logits_absmax = float(torch.nn.functional.conv2d(
            feats, wk.reshape(w.shape[0], -1, 1, 1), b).abs().max())
    out['bench_batch_random_network'] = dict(_parity_numbers(ours, ref, truth), logits_absmax=logits_absmax)
    out['mpjpe_mm'] = max(out['consistent_low']['mpjpe_mm'], out['consistent_peaked']['mpjpe_mm'])
    out['mpjpe_mm_is'] = 'the larger MPJPE of the two consistent regimes (NOT of the timed batch)'
    out['max_abs_mm'] = max(out['consistent_low']['max_abs_mm'], out['consistent_peaked']['max_abs_mm'])
    out['max_abs_mm_is'] = ('the largest |ours - reference| over all coordinates in the two consistent regimes; read it '
                            'against reference_run_to_run_max_mm, the reference\'s own spread between runs on the same '
                            'inputs (torch.linalg.lstsq / threaded conv; tests/golden/parity_reference_jitter.json)')
    out['consistent_regimes_within_1e-3_mm'] = bool(out['mpjpe_mm'] <= 1e-3)
    out['timed_batch_mpjpe_mm'] = out['bench_batch_random_network']['mpjpe_mm']
    out['timed_batch_within_1e-3_mm'] = bool(out['timed_batch_mpjpe_mm'] <= 1e-3)
    out['timed_batch_note'] = ('the batch the bench timed comes from a random-weight network: nearly uniform '
                               'heatmaps, reference-point depth ill-conditioned; ours_vs_fp64 / ref_vs_fp64 in '
                               'bench_batch_random_network show whose rounding the distance is')
    return out


def parity_from_identical_crops(est, extras, cfg, args):
    """The north star's literal sentence: "match the reference metrabs_pytorch CPU path on identical 256x256
    crops".  The SAME crops (the first n of the batch the bench just sampled) go through
      ours: the GPU backbone exactly as the step runs it (PyTorch-ROCm: MIOpen / rocBLAS, batch norm folded,
            K10 / K11 epilogues) -> mtr_head_fused -> mtr_reconstruct_absolute;
      ref:  the network as the reference runs it on the CPU (oneDNN, batch norms as ops) -> oracle/cpu_ref.py.
    The head is a PLAUSIBLE-POSE head for these features (cases.consistent_head_for_features: least-squares
    weights under which the CPU backbone's features of these crops decode to a person 2.5 - 4.5 m away --
    n <= C / (h w) crops), so the distance is read on well-conditioned poses.  Reported, not gated: it is
    dominated by the out-of-scope backbone (MIOpen vs oneDNN arithmetic through ~40 layers, times the head's
    gain); `head_on_reference_features` is the same comparison with the CPU features fed to our head -- the
    in-scope part."""
    from oracle import cases, cpu_ref
    from metrabs_amd import kernels
    model = est.crop_model
    J, D, P = model.joint_info.n_joints, cfg.depth, cfg.proc_side
    C = model.backbone.out_channels
    side = args.res // 32
    n = max(1, min(16, C // (side * side), len(extras['crops'])))
    crops = extras['crops'][:n].float()
    ocfg = cpu_ref.HeadConfig(proc_side=P, depth=D)
    backbone_cpu = copy.deepcopy(getattr(est, 'reference_backbone', model.backbone)).to('cpu', torch.float32).eval()
    with torch.inference_mode():
        feats_cpu = backbone_cpu(crops.cpu())
        w, b, K = cases.consistent_head_for_features(feats_cpu, J, D, P, amp=12.0, seed=515)
        ref = cpu_ref.crop_model_from_features(feats_cpu, w, b, K, J, ocfg)
        truth = cpu_ref.crop_model_from_features_fp64(feats_cpu, w, b, K, J, ocfg)
        logits_absmax = float(torch.nn.functional.conv2d(feats_cpu, w[:, :, None, None], b).abs().max())
        if model.autocast_dtype is not None:
            with torch.autocast('cuda', dtype=model.autocast_dtype):
                feats_gpu = model.backbone(extras['crops'][:n])
        else:
            feats_gpu = model.backbone(extras['crops'][:n])
        packed = kernels.head_pack_weights(w.cuda(), b.cuda(), J, D, feats_gpu.dtype)
        ours = kernels.reconstruct_absolute(*kernels.head_fused(feats_gpu, packed, C, J, model.config), K.cuda(),
                                            model.config).cpu()
        f_as = feats_cpu.cuda().to(feats_gpu.dtype)
        packed_ref = kernels.head_pack_weights(w.cuda(), b.cuda(), J, D, f_as.dtype)
        head_only = kernels.reconstruct_absolute(*kernels.head_fused(f_as, packed_ref, C, J, model.config), K.cuda(),
                                                 model.config).cpu()
    fd = (feats_gpu.float().cpu() - feats_cpu).abs()
    return dict(crops=n, mpjpe_mm=cpu_ref.mpjpe(ours, ref), max_abs_mm=float((ours - ref).abs().max()),
                head_on_reference_features=dict(mpjpe_mm=cpu_ref.mpjpe(head_only, ref),
                                                max_abs_mm=float((head_only - ref).abs().max()),
                                                ours_vs_fp64_mpjpe_mm=cpu_ref.mpjpe(head_only, truth),
                                                ref_vs_fp64_mpjpe_mm=cpu_ref.mpjpe(ref, truth)),
                backbone_features=dict(max_abs_diff=float(fd.max()), mean_abs_diff=float(fd.mean()),
                                       reference_abs_mean=float(feats_cpu.abs().mean()),
                                       gpu_dtype=str(feats_gpu.dtype).split('.')[-1]),
                logits_absmax=logits_absmax, median_depth_mm=float(truth[..., 2].median()),
                gated=False,
                note='ours (GPU backbone as the step runs it + HIP head + reconstruction) vs the CPU path on the '
                     'SAME crops, plausible-pose head fitted to the CPU features; the distance is the out-of-scope '
                     'backbone\'s (MIOpen vs oneDNN) times the head\'s gain -- head_on_reference_features is the '
                     'in-scope part on identical features')


DUMP_LIMIT_BYTES = 64 << 20


def step_outputs(api_result, pipe, strong, shard_out, gathered):
    """What the caller of the timed path received in the last step (rank 0's view): the API's poses,
    concatenated over the frames, or the captured pipeline's output buffers; plus the all-gathered poses
    of the job when the step ends in a collective."""
    if api_result is not None:
        out = {'poses3d': torch.cat(api_result['poses3d']), 'poses2d': torch.cat(api_result['poses2d'])}
    elif strong:
        out = {'poses3d': shard_out}
    else:
        out = {'poses3d': pipe.poses3d, 'poses2d': pipe.poses2d}
    if gathered is not None:
        out['poses3d_all_ranks'] = gathered
    torch.cuda.synchronize()
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def dump_outputs(directory, arrays):
    """DIR/<name>.npy, float32 (float64 stays float64).  Over 64 MB in all, a fixed, seeded sample of rows."""
    os.makedirs(directory, exist_ok=True)
    total = sum(v.numel() * (8 if v.dtype == torch.float64 else 4) for v in arrays.values())
    for name, v in arrays.items():
        a = v.numpy().astype(np.float64 if v.dtype == torch.float64 else np.float32)
        if total > DUMP_LIMIT_BYTES and a.shape[0] > 1:
            keep = max(1, int(a.shape[0] * DUMP_LIMIT_BYTES // total))
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], keep, replace=False))]
        np.save(os.path.join(directory, name + '.npy'), a)


def spawn_ranks(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: start the N ranks here --
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py <same arguments>`, one process per GPU (rank r on cuda:r, backend nccl
    = RCCL over xGMI) -- and hand its exit code on.  Fails loudly when the node has fewer than N
    GPUs: a line with n_gpus < N for a --gpus N command is never printed.
    MTR_BENCH_SHARED_DEVICE=1: all ranks on cuda:0 over gloo -- only to exercise the N > 1 code
    path on a 1-GPU box (RCCL refuses two ranks on one device)."""
    import socket
    import subprocess
    shared = os.environ.get('MTR_BENCH_SHARED_DEVICE') == '1'
    have = torch.cuda.device_count()
    if not shared and have < args.gpus:
        raise SystemExit(f'bench.py --gpus {args.gpus}: this node has {have} GPU(s); refusing to measure fewer '
                         f'ranks than asked for (MTR_BENCH_SHARED_DEVICE=1 runs the N-rank code path on '
                         f'one device for testing)')
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        port = sock.getsockname()[1]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')  # dmabuf IPC: what RCCL needs on this stack
    env.setdefault('OMP_NUM_THREADS', '1')
    if shared:
        env.setdefault('MTR_BENCH_BACKEND', 'gloo')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}',
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print('bench.py: starting', args.gpus, 'ranks:', ' '.join(cmd), file=sys.stderr)
    raise SystemExit(subprocess.call(cmd, env=env))


def main():
    args = parse_args()
    from metrabs_amd import distributed
    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs a GPU (the hot path has no CPU fallback)')
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ and 'RANK' not in os.environ:
        spawn_ranks(args)  # (does not return)
    # stdout carries ONE JSON line and nothing else: whatever native code writes to file descriptor 1
    # (RCCL prints its version banner there; MIOpen now and then) goes to stderr instead
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)
    sys.stdout = os.fdopen(json_fd, 'w')
    # one process per GPU; the device is bound BEFORE the process group exists so that RCCL's
    # communicator and barriers land on it.  MTR_BENCH_SHARED_DEVICE=1 (+ MTR_BENCH_BACKEND=gloo)
    # lets several ranks share cuda:0 -- only to exercise the N>1 code path on a 1-GPU box.
    local_rank = int(os.environ.get('LOCAL_RANK', os.environ.get('RANK', '0')))
    shared_device = os.environ.get('MTR_BENCH_SHARED_DEVICE') == '1'
    if shared_device:
        local_rank = 0
    world_env = int(os.environ.get('WORLD_SIZE', '1'))
    if world_env != args.gpus:
        raise SystemExit(f'bench.py --gpus {args.gpus} was started with WORLD_SIZE={world_env}: the launcher and '
                         f'--gpus disagree; refusing to print a line for a job of another size')
    if local_rank >= torch.cuda.device_count():
        raise SystemExit(f'bench.py: rank with LOCAL_RANK={local_rank} on a node with '
                         f'{torch.cuda.device_count()} GPU(s)')
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    force = bool(args.force_collective) and world_env == 1
    if force:
        import socket
        with socket.socket() as sock:
            sock.bind(('127.0.0.1', 0))
            os.environ.setdefault('MASTER_PORT', str(sock.getsockname()[1]))
    rank, world, _ = distributed.init_from_env(
        backend=os.environ.get('MTR_BENCH_BACKEND') or ('gloo' if shared_device and world_env > 1 else None),
        force_group=force, timeout_s=1800)
    collective = world > 1 or force   # the step ends in the all-gather of the poses
    from metrabs_amd import _lib
    from metrabs_amd.pipeline import GraphedCropPipeline
    _lib.load()

    est, cfg = build_model(args, dev)
    n_box = args.batch // args.num_aug
    im_h, im_w = 1080, 1920
    pipe = GraphedCropPipeline(est, args.frames, im_h, im_w, n_box, num_aug=args.num_aug,
                               use_graph=not args.no_graph)
    synth_inputs(pipe, args.frames, im_h, im_w, n_box, seed=100 + rank)
    full = args.full and not args.quick

    J = est.joint_info.n_joints
    # config 1 (weak scaling): one internal batch per rank and step.  config 2 (strong scaling): the
    # step's total crops form internal batches of args.batch crops, dealt round-robin to the ranks
    # (metrabs_amd.distributed.shard_internal_batches -- the unit of multiperson_model.py:189-220);
    # a rank replays its graph once per batch it owns, then the poses of the step are all-gathered.
    strong = args.strong
    # ---- the timed step of the weak-scaling configs goes through the drop-in API itself
    step_mode = args.step
    if step_mode == 'auto':
        step_mode = 'pipeline' if (strong or args.graph_gather or args.no_graph) else 'api'
    if step_mode == 'api' and strong:
        raise SystemExit('--step api: the strong-scaling configs replay one captured internal batch per owned batch')
    if step_mode == 'pipeline' or full:
        # (the API step captures its own graphs: the bare pipeline is timed, or compared against and probed
        #  by --full)
        pipe.capture()
    if strong:
        total_boxes = args.total_crops // args.num_aug
        my_batches = len(distributed.shard_internal_batches(total_boxes, n_box, rank, world))
        max_batches = len(distributed.shard_internal_batches(total_boxes, n_box, 0, world))
    else:
        my_batches = max_batches = 1
    gathered = torch.empty(world * max_batches * n_box, J, 3, device=dev) if collective else None
    shard_out = torch.zeros(max_batches * n_box, J, 3, device=dev) if strong else None

    use_base_gather = collective and torch.distributed.get_backend() == 'nccl'
    gather_mode = 'eager all_gather_into_tensor after the graph replay (outside the HIP graph)'
    graph_gather = False
    if args.graph_gather and use_base_gather and not strong and not args.no_graph:
        try:  # re-capture the step with the collective inside the graph
            pipe.after_step = lambda poses: torch.distributed.all_gather_into_tensor(gathered, poses.contiguous())
            pipe.capture()
            torch.cuda.synchronize()
            graph_gather = True
            gather_mode = 'all_gather_into_tensor captured inside the step\'s HIP graph (--graph-gather)'
        except Exception as e:  # noqa: BLE001 -- any capture failure: back to the eager gather
            pipe.after_step = None
            pipe.capture()
            gather_mode += f' [--graph-gather failed: {str(e)[:120]}]'

    api_call = None
    api_last = [None]   # the API's return value of the latest call (--dump-outputs)
    api_vs_pipeline_max_mm = None
    if step_mode == 'api':
        per_frame = [int((pipe.image_ids == i).sum()) for i in range(args.frames)]
        order = torch.argsort(pipe.image_ids.long(), stable=True)   # the API takes boxes frame by frame
        boxes_sorted = pipe.boxes[order].cpu()
        api_boxes = [b.numpy().copy() for b in torch.split(boxes_sorted, per_frame)]
        api_K = pipe.intrinsics[order].cpu()[torch.cumsum(torch.tensor([0] + per_frame[:-1]), 0)].numpy().copy()
        est.graph_batches = True
        api_kw = dict(intrinsic_matrix=api_K, internal_batch_size=n_box * args.num_aug, num_aug=args.num_aug)
        # every step gets ANOTHER set of frames (six sets in HBM, 300 MB at 8 x 1080p: more than the 256 MB
        # Infinity Cache), so no step finds its frames where the previous one left them
        gf = torch.Generator().manual_seed(4000 + rank)
        frame_sets = [pipe.images] + [torch.randint(0, 256, tuple(pipe.images.shape), dtype=torch.uint8,
                                                    generator=gf).to(dev) for _ in range(5)]
        api_turn = [0]

        def api_call():
            frames_now = frame_sets[api_turn[0] % len(frame_sets)]
            api_turn[0] += 1
            res = est.estimate_poses_batched(frames_now, api_boxes, **api_kw)
            api_last[0] = res
            return torch.cat(res['poses3d'])

        with torch.inference_mode():
            first = api_call()
            if full:
                # the API's internal batch is the pipeline's: same kernels, same shapes, same box order (synth_inputs
                # lays the boxes out frame by frame) -- the difference is reported in the line, 0.0 expected
                want = pipe.run()[order]
                api_vs_pipeline_max_mm = float((first - want).abs().max())
            if not torch.isfinite(first).all():
                raise SystemExit('bench: non-finite poses from the API step')

    def step():
        if api_call is not None:
            with torch.inference_mode():
                poses = api_call()
        elif strong:
            for b in range(my_batches):
                shard_out[b * n_box:(b + 1) * n_box].copy_(pipe.run(), non_blocking=True)
            poses = shard_out
        else:
            poses = pipe.run()
        if collective and not graph_gather:
            # the single collective of the path: KB-sized all-gather of the poses over RCCL/xGMI
            if use_base_gather:
                torch.distributed.all_gather_into_tensor(gathered, poses.contiguous())
            else:  # gloo (test harness only: two ranks sharing a GPU): through the host -- gloo's own
                # CUDA path stalls for tens of seconds now and then when its input is still being
                # written by a graph replay (tools/experiments/n2_debug2.py)
                host = poses.contiguous().cpu()
                parts = [torch.empty_like(host) for _ in range(world)]
                torch.distributed.all_gather(parts, host)
                gathered.copy_(torch.cat(parts), non_blocking=True)

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if collective:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    if collective:
        torch.distributed.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, step_outputs(api_last[0], pipe, strong, shard_out, gathered))
    multi = None
    if collective:
        # every rank's own time for the K steps (one line must be enough to diagnose a flat curve),
        # then the max over ranks = the job's time; the gather alone, timed on its own afterwards
        mine = torch.tensor([elapsed], dtype=torch.float64, device=dev if use_base_gather else 'cpu')
        per_rank = [torch.empty_like(mine) for _ in range(world)]
        torch.distributed.all_gather(per_rank, mine)
        per_rank = [float(t.item()) for t in per_rank]
        elapsed = max(per_rank)
        n_g = max(10, args.steps)
        poses_now = (shard_out if strong else (api_call() if api_call is not None else pipe.poses)).contiguous()
        torch.cuda.synchronize()
        torch.distributed.barrier()
        tg = time.perf_counter()
        for _ in range(n_g):
            if use_base_gather:
                torch.distributed.all_gather_into_tensor(gathered, poses_now)
            else:
                host = poses_now.cpu()
                parts = [torch.empty_like(host) for _ in range(world)]
                torch.distributed.all_gather(parts, host)
        torch.cuda.synchronize()
        gather_us = (time.perf_counter() - tg) / n_g * 1e6
        multi = dict(per_rank_ms_per_step=[round(t / args.steps * 1e3, 4) for t in per_rank],
                     gather_us_per_step_alone=round(gather_us, 1),
                     gather_bytes_per_rank=int(poses_now.numel() * 4),
                     backend=torch.distributed.get_backend(), world_size=world,
                     gathered_equals_poses=bool(torch.equal(
                         gathered.reshape(world, -1, J, 3)[rank][:poses_now.shape[0]], poses_now)) if use_base_gather
                     else None,
                     devices='all ranks on cuda:0 (MTR_BENCH_SHARED_DEVICE=1: code-path test, not a '
                             'scaling measurement)' if shared_device else (
                         'ONE rank (--force-collective: RCCL exercised on a 1-GPU box, not a scaling measurement)'
                         if force else 'one GPU per rank'),
                     gather=gather_mode)

    if rank != 0:
        if world > 1:
            # rank 0 runs its probes now (its line is printed BEFORE it joins this barrier); the process group was
            # made with a 30-minute timeout so that a slow probe cannot trip the collective watchdog here
            try:
                torch.distributed.barrier()
                torch.distributed.destroy_process_group()
            except Exception as e:  # noqa: BLE001
                print(f'bench.py: rank {rank}: final barrier failed:', repr(e)[:200], file=sys.stderr)
        return

    crops_per_step = args.total_crops if strong else world * n_box * args.num_aug
    value = crops_per_step * args.steps / elapsed

    workload = {
        1: f'configs[1]: {args.backbone} {args.res}px, batch {n_box * args.num_aug} crops/GPU, ',
        2: f'configs[2]: {args.backbone} {args.res}px, {args.total_crops} crops/step in internal batches of '
           f'{n_box * args.num_aug} dealt round-robin to {world} rank(s), ',
        3: f'configs[3]: {args.backbone} {args.res}px, {args.frames} frames x {n_box // max(args.frames, 1)} boxes x '
           f'num_aug {args.num_aug} (rotations, scales, flips, gammas of multiperson_model.py:108-137) = '
           f'{n_box * args.num_aug} crops/GPU as one internal batch, ',
        4: f'configs[4]: {args.backbone} {args.res}px under {args.precision} autocast, {J}-joint head, '
           f'{args.total_crops} crops/step in internal batches of {n_box * args.num_aug} dealt round-robin to '
           f'{world} rank(s), ',
    }[args.config]
    out = {
        # BASELINE.json's metric string, verbatim.  NB its "72 depth bins": the reference default
        # and every shipped config use depth=8, which is what runs here; the
        # same step with a 72-bin head rides along as `depth72`.
        'metric': 'crops/sec (256px, 72 depth bins) at 1/2/4/8 MI355X; MPJPE vs ref',
        'value': value, 'unit': 'crops/s', 'n_gpus': world, 'steps': args.steps,
        'warmup': args.warmup, 'ms_per_step': elapsed / args.steps * 1e3,
        'higher_is_better': True, 'scaling': 'strong' if strong else 'weak', 'vs_baseline': None,
        'dtype': args.precision, 'data': 'synthetic',
        'config': {'workload': workload + f'num_aug={args.num_aug}, {args.frames} 1080p uint8 frames per internal '
                                          f'batch, J={J}, D={cfg.depth} depth bins (every shipped configuration of the '
                                          f'reference; the metric string\'s 72-bin reading of the same step is the '
                                          f'`depth72` object of this line), random weights',
                   'global_batch': crops_per_step, 'parallelism': f'dp{world} (crops sharded, one '
                   f'all-gather of poses)' if world > 1 else 'single GPU',
                   'hip_graph': not args.no_graph,
                   'step_through': ('Pose3dEstimator.estimate_poses_batched(frames on the device, host boxes and '
                                    'cameras) with the estimator\'s own HIP-graph cache (graph_batches=True): per step '
                                    'the host camera set-up, one pinned upload of the per-box parameters, the frames '
                                    'copied into the sampler\'s buffer, the pyramid, one graph launch, the result '
                                    'cloned out and split per frame; six frame sets (300 MB) in rotation, a step never '
                                    'sees the frames of the one before' if step_mode == 'api' else
                                    'a bare replay of the captured internal batch (metrabs_amd.pipeline.'
                                    'GraphedCropPipeline) on static inputs'),
                   'api_step_vs_captured_pipeline_max_mm': api_vs_pipeline_max_mm if step_mode == 'api' else None,
                   'deterministic_backbone': bool(est.crop_model.backbone_is_pinned()),
                   'backbone': 'PyTorch-ROCm (dense convolutions on rocBLAS / MIOpen' + (
                       '; depthwise layers on PyTorch\'s own kernel' if args.no_fold_bn else
                       '; inference batch norm folded into the convolutions' + (
                           '; depthwise layers on PyTorch\'s own kernel' if args.no_fused_epilogue else
                           '; bias + activation (+ skip connection, + squeeze-excite mean) behind them as '
                           'one in-place HIP pass (K10); depthwise 3x3 layers with that epilogue in one '
                           'HIP pass (K11)')) + ')'},
    }
    if multi is not None:
        out['multi_gpu'] = multi
    if not full:
        out.update(roofline=None, cpu_baseline=None,
                   note='the contract line only (per-kernel timing, probes, variants and baselines: --full)')
    else:
        try:
            out.update(analysis(args, est, cfg, pipe, dev, elapsed / args.steps, im_h, im_w, n_box, world))
        except BaseException as e:  # noqa: BLE001 -- the contract line survives whatever the probes do
            out.setdefault('roofline', None)
            out.setdefault('cpu_baseline', None)
            out['analysis_error'] = repr(e)[:400]
            if isinstance(e, KeyboardInterrupt):
                print(json.dumps(out))
                sys.stdout.flush()
                raise
    print(json.dumps(out))
    sys.stdout.flush()
    if collective:
        try:  # the line is out: a peer that gave up waiting must not turn the run's exit code red
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
        except Exception as e:  # noqa: BLE001
            print('bench.py: final barrier failed after the line was printed:', repr(e)[:200], file=sys.stderr)


def pcie_variants(pipe, args, n_box):
    """NOT `value`: the frames arrive from pinned host memory every step -- blocking, and with the
    copy of step i + 1 on its own stream under the compute of step i (two staging buffers in HBM,
    one device-to-device copy into the graph's input per step)."""
    host_frames = pipe.images.cpu().pin_memory()
    n_pcie = max(5, args.steps // 3)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(n_pcie):
        pipe.images.copy_(host_frames, non_blocking=True)
        pipe.run()
    torch.cuda.synchronize()
    pcie_ms = (time.perf_counter() - t1) / n_pcie * 1e3
    assert torch.isfinite(pipe.poses).all(), 'non-finite poses in the benchmark step'
    copy_stream = torch.cuda.Stream()
    staging = [torch.empty_like(pipe.images) for _ in range(2)]
    ready = [torch.cuda.Event() for _ in range(2)]
    free = [torch.cuda.Event() for _ in range(2)]
    cur = torch.cuda.current_stream()
    with torch.cuda.stream(copy_stream):
        staging[0].copy_(host_frames, non_blocking=True)
        ready[0].record(copy_stream)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    for i in range(n_pcie):
        b = i & 1
        with torch.cuda.stream(copy_stream):
            if i >= 1:
                copy_stream.wait_event(free[b ^ 1])
            staging[b ^ 1].copy_(host_frames, non_blocking=True)
            ready[b ^ 1].record(copy_stream)
        cur.wait_event(ready[b])
        pipe.images.copy_(staging[b], non_blocking=True)
        free[b].record(cur)
        pipe.run()
    torch.cuda.synchronize()
    pcie_ovl_ms = (time.perf_counter() - t2) / n_pcie * 1e3
    assert torch.isfinite(pipe.poses).all(), 'non-finite poses in the benchmark step'
    crops = n_box * args.num_aug
    return {'ms_per_step': pcie_ms, 'crops_per_s_per_gpu': crops / (pcie_ms * 1e-3),
            'note': f'{args.frames} uint8 1080p frames ({pipe.images.numel() / 1e6:.1f} MB) copied '
                    'from pinned host memory before every step; not part of `value`',
            'overlapped': {'ms_per_step': pcie_ovl_ms, 'crops_per_s_per_gpu': crops / (pcie_ovl_ms * 1e-3),
                           'note': 'the copy of step i+1 runs on its own HIP stream under '
                                   'the compute of step i (two staging buffers in HBM)'}}


def api_path_probe(est, args, im_h, im_w, n_box, value):
    """crops/s through ``Pose3dEstimator.estimate_poses_batched`` -- the drop-in surface itself
    (multiperson_model.py:62-74,184-225 of the reference), not the bench's fixed-shape pipeline object:
    every call builds its cameras and per-box parameters on the host from FRESH host arrays (boxes,
    intrinsics), uploads them, copies the call's frames into the sampler's buffer, builds the pyramid and
    runs the internal batch -- eagerly (graph_batches=False) or through the estimator's shape-bucketed
    HIP-graph cache (graph_cache.py).  Frames: device-resident uint8 tensors as the reference's own demo
    feeds them (scripts/demo_image.py:34), six different sets in rotation (300 MB, more than the 256 MB
    Infinity Cache), and pinned host tensors.  `full`: 8 boxes on each of the 8 frames = the step of
    `value`; `ragged`: 1 - 8 boxes per frame, every call another count (a graph per distinct batch size,
    all captured before the timed calls)."""
    frames = args.frames
    per = max(n_box // frames, 1)
    g = torch.Generator().manual_seed(7)
    rng = np.random.default_rng(7)
    dev_sets = [torch.randint(0, 256, (frames, 3, im_h, im_w), dtype=torch.uint8, generator=g).cuda()
                for _ in range(6)]
    host_sets = [d.cpu().pin_memory() for d in dev_sets[:2]]
    f = max(im_h, im_w) / (np.tan(np.deg2rad(55.0) / 2) * 2)
    K0 = np.array([[f, 0, im_w / 2], [0, f, im_h / 2], [0, 0, 1]], np.float32)

    def fresh_call(counts):
        boxes = []
        for n in counts:
            bw = 60 + 340 * rng.random(n)
            bh = 150 + 750 * rng.random(n)
            bx = rng.random(n) * (im_w - bw)
            by = rng.random(n) * np.maximum(im_h - bh, 1.0)
            boxes.append(np.stack([bx, by, bw, bh], axis=1).astype(np.float32))
        K = np.repeat(K0[None], frames, axis=0) * (1 + 0.01 * rng.standard_normal((frames, 1, 1)).astype(np.float32))
        K[:, 2, 2] = 1.0
        return boxes, K

    def timed(mode, image_sets, calls, rounds):
        est.graph_batches = mode
        est.graphs.max_graphs = 80
        inputs = [fresh_call(c) for c in calls]
        kw = dict(internal_batch_size=n_box * args.num_aug, num_aug=args.num_aug)
        for _ in range(2):  # every batch size seen (and, graphed, captured) before the timed calls
            for i, (boxes, K) in enumerate(inputs):
                est.estimate_poses_batched(image_sets[i % len(image_sets)], boxes, intrinsic_matrix=K, **kw)
        torch.cuda.synchronize()
        n_crops, t0 = 0, time.perf_counter()
        for r in range(rounds):
            for i, c in enumerate(calls):
                boxes, K = fresh_call(c)   # (host arrays made inside the timed region: part of a call's cost)
                res = est.estimate_poses_batched(image_sets[(r + i) % len(image_sets)], boxes, intrinsic_matrix=K, **kw)
                n_crops += sum(c) * args.num_aug
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert all(torch.isfinite(p).all() for p in res['poses3d'])
        lat = []   # one call at a time, the host waiting for its result: what a live camera loop sees
        for i, c in enumerate(calls[:6]):
            boxes, K = fresh_call(c)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            res = est.estimate_poses_batched(image_sets[i % len(image_sets)], boxes, intrinsic_matrix=K, **kw)
            res['poses3d'][0].cpu()
            lat.append((time.perf_counter() - t1) * 1e3)
        return dict(crops_per_s=round(n_crops / dt, 1), ms_per_call=round(dt / (rounds * len(calls)) * 1e3, 3),
                    calls=rounds * len(calls), crops_per_call=round(n_crops / (rounds * len(calls)), 1),
                    latency_ms_one_call_synced=round(float(np.median(lat)), 3))

    full = [[per] * frames] * 6
    ragged = [list(rng.integers(1, per + 1, frames)) for _ in range(16)]
    rounds = max(2, args.steps // 10)
    before = (est.graph_batches, est.graphs.max_graphs)
    out = {}
    try:
        with torch.inference_mode():
            out['full'] = dict(eager=timed(False, dev_sets, full, rounds), graphed=timed(True, dev_sets, full, rounds),
                               eager_frames_from_pinned_host=timed(False, host_sets, full, rounds),
                               graphed_frames_from_pinned_host=timed(True, host_sets, full, rounds))
            out['ragged_1_to_%d_boxes_per_frame' % per] = dict(eager=timed(False, dev_sets, ragged, 2),
                                                               graphed=timed(True, dev_sets, ragged, 2))
            # the live-camera case: ONE 1080p frame with one / four boxes per call, the host waiting for every result
            # (launch-bound when eager: ~400 launches for a batch the GPU finishes in a fraction of their issue time)
            small = {}
            for n_b in (1, 4):
                one_frame = [d[:1] for d in dev_sets]
                res_mode = {}
                for mode in (False, True):
                    est.graph_batches = mode
                    lat = []
                    for i in range(12):
                        bw = 60 + 340 * rng.random(n_b)
                        bh = 150 + 750 * rng.random(n_b)
                        bx = rng.random(n_b) * (im_w - bw)
                        by = rng.random(n_b) * np.maximum(im_h - bh, 1.0)
                        boxes = [np.stack([bx, by, bw, bh], axis=1).astype(np.float32)]
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        res = est.estimate_poses_batched(one_frame[i % len(one_frame)], boxes, intrinsic_matrix=K0[None],
                                                         internal_batch_size=n_box * args.num_aug, num_aug=args.num_aug)
                        res['poses3d'][0].cpu()
                        lat.append((time.perf_counter() - t1) * 1e3)
                    res_mode['graphed' if mode else 'eager'] = round(float(np.median(lat[4:])), 3)
                small[f'{n_b}_box'] = dict(latency_ms_one_call_synced=res_mode,
                                           speedup=round(res_mode['eager'] / res_mode['graphed'], 2))
            out['one_frame_per_call'] = small
            out['graph_cache'] = dict(est.graphs.stats, graphs=len(est.graphs.graphs))
    finally:
        est.graph_batches, est.graphs.max_graphs = before
        est.graphs.clear()
        torch.cuda.empty_cache()
    out['graphed_over_value'] = round(out['full']['graphed']['crops_per_s'] / value, 4)
    out['note'] = ('Pose3dEstimator.estimate_poses_batched(images, boxes, intrinsic_matrix=...) called back to back with '
                   'fresh host boxes / cameras per call; `value` is the same internal batch as a bare graph replay on '
                   'static inputs')
    return out


def live_pmc_traffic(args, n_crops, J, D, C, timeout=240):
    """HBM-side bytes per launch of the step's hand-written kernels, measured NOW: two rocprofv3 passes
    (--pmc FETCH_SIZE, --pmc WRITE_SIZE; --kernel-trace only, one counter per pass as
    MI355X_MICROARCH.md prescribes: they do not fit one pass) over tools/_pmc_step.py, which launches
    the same kernels at the bench's shapes (sampler kernels on rotating frames).  bytes = FETCH_SIZE x 2
    (the guide's gfx950 correction for wide streaming reads) + WRITE_SIZE.  -> (dict by kernel,
    source string) or (None, reason)."""
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which('rocprofv3') or '/opt/rocm/bin/rocprofv3'
    if not os.path.exists(exe):
        return None, 'rocprofv3 not found'
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from pmc_traffic import per_kernel_average
    cmd = [sys.executable, os.path.join(ROOT, 'tools', '_pmc_step.py'), str(n_crops), str(args.res),
           args.precision, str(J), str(D), str(C), str(args.frames), str(args.num_aug)]
    res = {}
    tmp = tempfile.mkdtemp(prefix='mtr_pmc_')
    env = dict(os.environ, TMPDIR='/tmp')
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT'):
        env.pop(k, None)
    try:
        for counter in ('FETCH_SIZE', 'WRITE_SIZE'):
            d = os.path.join(tmp, counter)
            try:
                r = subprocess.run([exe, '--pmc', counter, '--kernel-trace', '--output-format', 'csv', '-d', d,
                                    '-o', 'p', '--'] + cmd, cwd='/tmp', env=env, capture_output=True, text=True,
                                   timeout=timeout)
            except subprocess.TimeoutExpired:
                return None, f'rocprofv3 --pmc {counter} pass exceeded {timeout} s'
            if r.returncode != 0:
                return None, f'rocprofv3 --pmc {counter} pass failed: {(r.stderr or r.stdout)[-300:]}'
            res[counter] = per_kernel_average(d, counter)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    out = {}
    for name in set(res['FETCH_SIZE']) | set(res['WRITE_SIZE']):
        f_kib, n_f = res['FETCH_SIZE'].get(name, (0.0, 0))
        w_kib, n_w = res['WRITE_SIZE'].get(name, (0.0, 0))
        out[name] = dict(bytes=int(round(f_kib * 2048 + w_kib * 1024)), fetch_KiB_raw=round(f_kib, 1),
                         write_KiB=round(w_kib, 1), launches_in_pass=max(n_f, n_w))
    return out, ('measured in this run: rocprofv3 --pmc FETCH_SIZE and --pmc WRITE_SIZE (--kernel-trace, one '
                 'counter per pass) over tools/_pmc_step.py at the bench shapes; bytes = FETCH_SIZE x 2 '
                 '(gfx950 correction, MI355X_MICROARCH.md) + WRITE_SIZE')


def analysis(args, est, cfg, pipe, dev, step_seconds, im_h, im_w, n_box, world):
    """Everything in the line besides the contract fields (rank 0, after the timed region).
    Round 6: `roofline` and `cpu_baseline` are computed FIRST and every other probe runs
    inside its own try / except that writes `<probe>_error` into the line -- no probe can lose the line (at N > 1
    the other ranks wait at the final barrier meanwhile)."""
    J = est.joint_info.n_joints
    out = {}

    fail = set(filter(None, os.environ.get('MTR_BENCH_FAIL_PROBE', '').split(',')))   # (tests: make a probe raise)

    def probe(key, fn, default=None):
        try:
            if key in fail:
                raise RuntimeError(f'MTR_BENCH_FAIL_PROBE names {key}')
            return fn()
        except Exception as e:  # noqa: BLE001 -- a reported number, never a reason to lose the line
            import traceback
            out[key + '_error'] = (repr(e)[:300] + ' @ ' + ' <- '.join(
                f'{os.path.basename(fr.filename)}:{fr.lineno}' for fr in traceback.extract_tb(e.__traceback__)[-3:]))
            return default

    try:
        core = _roofline_analysis(args, est, cfg, pipe, dev, step_seconds, im_h, im_w, n_box, world, out, probe)
    except Exception as e:  # noqa: BLE001
        out['roofline'] = None
        out['roofline_error'] = repr(e)[:400]
        core = None
    if world == 1 and not args.no_cpu_baseline:
        out['cpu_baseline'] = probe('cpu_baseline', lambda: cpu_baseline(est, pipe, args, cfg, args.cpu_seconds))
    else:
        out['cpu_baseline'] = None
    if core is not None:
        _secondary_probes(args, est, cfg, pipe, dev, step_seconds, im_h, im_w, n_box, world, out, probe, core)
    return out


def _roofline_analysis(args, est, cfg, pipe, dev, step_seconds, im_h, im_w, n_box, world, out, probe):
    """Per-stage timing, the roofline object of the dominant section-8 kernel, the per-kernel table."""
    J = est.joint_info.n_joints
    # ---- per-stage timing + roofline of the dominant hand-written kernel of SURVEY section 8
    iters = max(10, args.steps)
    stages, extras = stage_breakdown(pipe, est, args, iters=iters)
    C = est.crop_model.backbone.out_channels
    hw = (args.res // 32) ** 2
    D = cfg.depth
    feat_bytes = 2 if args.precision != 'f32' else 4
    out_bytes = 2 if args.precision != 'f32' else 4
    n_crops = n_box * args.num_aug
    # pyramid: read the uint8 frames, write f32 levels 1 and 2 (level 0 stays uint8 + LUT)
    pyr_bytes = args.frames * 3 * (im_h * im_w * 1 + (im_h // 2) * (im_w // 2) * 4 +
                                   (im_h // 4) * (im_w // 4) * 4)
    src_bytes = source_footprint_bytes(extras['wp'], args.res, im_h, im_w)
    head_flops = 2.0 * C * J * (1 + D) * hw * n_crops
    heads = est.crop_model.heatmap_heads
    head_is_fused = heads.last_path == 'fused'
    head_kernel = head_kernel_name(hw, n_crops, J, D, args.precision, C) if head_is_fused else \
        'library 1x1 conv (rocBLAS / MIOpen) + decode_nchw_kernel'
    # f32 features: f32-input MFMA (f64 carry on the VALU), matrix-bound.  16-bit features: f16 / bf16
    # MFMA at 16x that rate -- the kernel is bounded by the feature bytes it stages
    h16 = args.precision != 'f32'
    mfma_peak = MFMA_F16_PEAK if h16 else MFMA_F32_PEAK
    rot = rotating_sampler_times(pipe, est, args, extras['wp'], iters)
    # every hand-written kernel of the step: launches per step, seconds per step, algorithmic bytes
    # (and flops) per step.  Sampler kernels: timed on rotating frames (HBM-true); `hot_us` is the
    # same launch on the step's own, cache-resident frames.
    hw_kernels = {
        'pyramid': dict(kernel='build_pyramid_u8_wide_kernel', bound='hbm', launches=1,
                        seconds=rot['pyramid'], bytes=pyr_bytes, hot_us=stages['pyramid'] * 1e6),
        'warp': dict(kernel='warp_rows_kernel', bound='hbm', launches=1, seconds=rot['warp'],
                     bytes=n_crops * 3 * args.res ** 2 * out_bytes + src_bytes,
                     hot_us=stages['warp'] * 1e6),
        'head_fused': dict(kernel=head_kernel, launches=1,
                           seconds=stages['head_fused'], flops=head_flops,
                           bytes=n_crops * (C * hw * feat_bytes + 20 * J),
                           hot_us=stages['head_fused'] * 1e6),
    }
    # the head is matrix-bound for f32 features (76 FLOP/B against a ridge of ~20) and for
    # J = 122 in any dtype (1098 FLOP/B of f16 features against 2.5 PF / 8 TB/s = 312); HBM-bound for 16-bit
    # features at J = 17 (153 FLOP/B).  Decided by the shape's own intensity, not by the dtype alone.
    hk = hw_kernels['head_fused']
    hk['flop_per_byte'] = hk['flops'] / hk['bytes']
    hk['bound'] = 'mfma' if hk['flop_per_byte'] > mfma_peak / HBM_PEAK else 'hbm'
    # the dominant kernel of the step AMONG THE ROWS OF SURVEY section 8 (head, sampler, pyramid), by
    # the time it takes inside the step; the backbone epilogues K10 / K11 are outside that scope and
    # stay in `hand_written_kernels`
    # "inside the step" = the in-step (hot) durations: the sampler runs right behind the pyramid kernel on the same
    # frames, i.e. on data the pyramid pass just pulled through the Infinity Cache -- the kernel trace of this very
    # command reads 21 - 24 us for it, not the 31 - 32 us of the sampler alone on rotating frames (which is what its
    # `frac_hbm` is quoted on).  Head and sampler sit within ~0.1 us of each other at configs[1] and the choice
    # flipped from box to box: within 5 % the head (the kernel rounds 1 - 4 reported) keeps the slot.
    in_step_us = lambda k: hw_kernels[k]['hot_us']
    dominant = max(hw_kernels, key=in_step_us)   # the true argmax (no tie-break towards the head)
    tie_within_5pct = [k for k in hw_kernels if k != dominant and in_step_us(k) >= 0.95 * in_step_us(dominant)]
    epilogue_hot = 0.0
    if not args.no_fold_bn and not args.no_fused_epilogue:
        for name, e in (probe('backbone_epilogue_kernels',
                              lambda: backbone_epilogue_kernels(est, extras['crops'], iters)) or {}).items():
            hw_kernels['K10 ' + name if name.startswith('bias') else 'K11 ' + name] = dict(
                kernel=name, bound='hbm', launches=e['launches_per_step'], seconds=e['seconds_per_step'],
                bytes=e['bytes_per_step'], slowest_launch=e['slowest'],
                hot_us=e['hot_seconds_per_step'] * 1e6)
            epilogue_hot += e['hot_seconds_per_step']
    small = {k: stages[k] for k in ('geometry', 'reconstruct', 'postprocess')}
    # share of the step spent in hand-written HIP: every kernel at its IN-STEP duration (inputs as
    # hot as the step leaves them), not at the rotating-buffer duration the fractions are quoted on
    ours_seconds = sum(v['hot_us'] * 1e-6 for v in hw_kernels.values()) + sum(small.values())
    a = hw_kernels[dominant]
    if a['bound'] == 'hbm':
        achieved, peak, unit = a['bytes'] / a['seconds'], HBM_PEAK, 'GB/s'
    else:
        achieved, peak, unit = a['flops'] / a['seconds'], mfma_peak, 'TFLOP/s'
    scale = 1e9 if unit == 'GB/s' else 1e12
    # HBM-side bytes per launch: measured in this run by two rocprofv3 --pmc passes; the stored file
    # of the round's profile set is only a labelled fallback
    tjson, traffic_source = None, None
    if not args.no_pmc and world == 1:  # (N > 1: the other ranks wait at the final barrier meanwhile)
        tjson, traffic_source = probe('live_pmc_traffic', lambda: live_pmc_traffic(args, n_crops, J, D, C),
                                      (None, 'live_pmc_traffic raised: see live_pmc_traffic_error'))
    if tjson is None:
        live_failure = traffic_source
        tpath = os.path.join(ROOT, 'profiles', 'traffic.json')
        try:
            tjson = json.load(open(tpath))
            traffic_source = ('STORED, not measured in this run (' + str(live_failure or '--no-pmc / N > 1') + '): ' +
                              str(tjson.get('_source')))
        except (OSError, ValueError):
            tjson, traffic_source = {}, f'none ({live_failure})'
    base = a['kernel'].split('<')[0].split(' ')[0]
    entry = tjson.get(base)
    traffic = entry.get('bytes') if isinstance(entry, dict) else None
    roofline = dict(kernel=a['kernel'], bound=a['bound'], achieved=achieved / scale,
                    peak=peak / scale, unit=unit, frac=achieved / peak, traffic=traffic,
                    traffic_source=traffic_source,
                    launches_per_step=a['launches'], tie_within_5pct=[hw_kernels[k]['kernel'] for k in tie_within_5pct],
                    avg_launch_us=a['seconds'] / a['launches'] * 1e6,
                    us_per_step=a['seconds'] * 1e6,
                    algorithmic_bytes_per_launch=a['bytes'] / a['launches'],
                    note='the hand-written kernel of SURVEY section 8 with the most time per step (head, '
                         'sampler or pyramid; the backbone epilogues K10 / K11 are in hand_written_kernels); '
                         'achieved = algorithmic flops (bytes) of one launch / its average duration between '
                         'HIP events on the launch stream, launches inside a replayed HIP graph (sampler '
                         'kernels: on rotating frames > 256 MiB)')
    if 'flops' in a:
        roofline['algorithmic_flops_per_launch'] = a['flops'] / a['launches']
    # the runner-up among the section-8 kernels, with its own bound (head and sampler are within a few us of each
    # other at configs[1]: both are always in the line)
    second = sorted((k for k in ('pyramid', 'warp', 'head_fused') if k != dominant), key=in_step_us)[-1]
    b2 = hw_kernels[second]
    roofline['runner_up'] = dict(
        kernel=b2['kernel'], bound=b2['bound'], avg_launch_us=b2['seconds'] / b2['launches'] * 1e6,
        frac=(b2['bytes'] / b2['seconds'] / HBM_PEAK) if b2['bound'] == 'hbm' else (b2['flops'] / b2['seconds'] / mfma_peak))
    kernels_us = {k: round(v * 1e6, 2) for k, v in stages.items()}
    per_kernel = {}
    for k, a2 in hw_kernels.items():
        t = a2['seconds']
        per_kernel[k] = dict(kernel=a2['kernel'], launches_per_step=a2['launches'],
                             us_per_step=round(t * 1e6, 2), GBps=round(a2['bytes'] / t / 1e9, 1),
                             frac_hbm=round(a2['bytes'] / t / HBM_PEAK, 4))
        if 'flops' in a2:
            per_kernel[k]['TFLOPs'] = round(a2['flops'] / t / 1e12, 2)
            per_kernel[k]['frac_mfma'] = round(a2['flops'] / t / mfma_peak, 4)
        if k in ('pyramid', 'warp'):
            t_il = rot[k + '_interleaved']
            per_kernel[k]['interleaved_frames'] = dict(
                us_per_step=round(t_il * 1e6, 2), frac_hbm=round(a2['bytes'] / t_il / HBM_PEAK, 4),
                note='the same launch on [N,H,W,3] frames (channels_last: what a decoder hands over), sampled in '
                     'place with the planar path\'s bits; `value` and the roofline object use the reference\'s '
                     'planar [N,3,H,W] frames')
            per_kernel[k]['us_on_the_steps_own_cache_resident_frames'] = round(a2['hot_us'], 2)
            per_kernel[k]['frac_hbm_cache_assisted'] = round(a2['bytes'] / (a2['hot_us'] * 1e-6) / HBM_PEAK, 4)
        if k.startswith('K1'):
            per_kernel[k]['us_per_step_on_hot_activations'] = round(a2['hot_us'], 2)
        if 'slowest_launch' in a2:
            per_kernel[k]['slowest_launch'] = a2['slowest_launch']
        tr = tjson.get(a2['kernel'].split('<')[0].split(' ')[0])
        if isinstance(tr, dict) and tr.get('bytes'):
            per_kernel[k]['traffic_bytes_per_launch'] = tr['bytes']
            # the same fraction on the bytes the counters saw (sampler: the bounding-box definition of SURVEY
            # section 8(d) counts source texels a rotated crop's quad never touches)
            per_kernel[k]['frac_hbm_by_counter_bytes'] = round(tr['bytes'] * a2['launches'] / t / HBM_PEAK, 4)
    for k, v in small.items():
        per_kernel[k] = dict(us_per_step=round(v * 1e6, 2), bound='latency (KB of data)')
    if not args.quick:
        per_kernel['K9 detector_pre (in front of the step, not in the timed region)'] = probe(
            'detector_pre', lambda: detector_pre_probe(pipe, iters))
    out.update({
        'roofline': roofline,
        'head_path': {'ran': 'mtr_head_fused' if head_is_fused else 'library 1x1 conv + mtr_softargmax_decode',
                      'kernel': head_kernel, 'fused_setting': str(heads.fused),
                      'auto_choices': {str(k): ('fused' if v else 'library') for k, v in heads._auto_choice.items()}},
        'stage_us': kernels_us,
        'hand_written_kernels': per_kernel,
        'hip_share_of_step': ours_seconds / step_seconds,
        'hip_share_note': 'every hand-written kernel at its in-step duration (K10 / K11: each launch of the '
                          'forward replayed on ONE buffer set, i.e. on activations as hot as the convolution '
                          'in front leaves them), over the step time',
    })
    return dict(extras=extras, tjson=tjson, traffic_source=traffic_source, head_is_fused=head_is_fused, h16=h16,
                n_crops=n_crops)


def _secondary_probes(args, est, cfg, pipe, dev, step_seconds, im_h, im_w, n_box, world, out, probe, core):
    """Everything behind `roofline` and `cpu_baseline`, each probe guarded on its own."""
    extras, tjson, traffic_source = core['extras'], core['tjson'], core['traffic_source']
    pcie = out['pcie_inclusive'] = probe('pcie_inclusive', lambda: pcie_variants(pipe, args, n_box))
    if core['head_is_fused'] and not core['h16'] and not args.quick:
        out['head_by_launch_size'] = probe('head_by_launch_size', lambda: head_by_launch_size(est, args, core['n_crops']))
    if not args.no_decode_roofline:
        def decode_probes():
            d = {'decode_roofline': decode_roofline()}
            d['decode_roofline']['traffic'] = (tjson.get('decode_nchw_kernel') or {}).get('bytes')
            d['decode_roofline']['traffic_source'] = traffic_source
            if not args.quick:
                d['decode_roofline_nhwc'] = decode_roofline(nhwc=True)
                d['decode_roofline_nhwc']['j122_12x12_b2048'] = {
                    k: v for k, v in decode_roofline(nhwc=True, shape=(2048, 122, 8, 12)).items()
                    if k in ('achieved', 'frac', 'avg_launch_us', 'crops', 'bytes_per_crop')}
            return d
        out.update(probe('decode_roofline', decode_probes) or {})
    out['parity'] = probe('parity', lambda: parity_probe(est, extras, cfg, args))
    if world == 1 and not args.quick and out['parity'] is not None:
        out['parity']['from_identical_crops'] = probe(
            'parity_from_identical_crops', lambda: parity_from_identical_crops(est, extras, cfg, args))
    if world == 1 and not args.no_api_path and not args.strong:
        out['api_path'] = probe('api_path', lambda: api_path_probe(
            est, args, im_h, im_w, n_box, n_box * args.num_aug / step_seconds))
    if world == 1 and args.depth != 72 and not args.no_depth72 and args.config == 1:
        probe('variants', lambda: _variant_probes(args, est, dev, im_h, im_w, n_box, out))
    api = out.get('api_path')
    if api or pcie:
        out['deployable'] = dict(
            crops_per_s=(api['full']['graphed_frames_from_pinned_host']['crops_per_s'] if api else
                         pcie['overlapped']['crops_per_s_per_gpu']),
            what=('Pose3dEstimator.estimate_poses_batched with the frames of every call arriving from pinned host memory '
                  'over PCIe (copy stream under the previous call\'s compute), fresh boxes / cameras per call: '
                  'api_path.full.graphed_frames_from_pinned_host' if api else
                  'pcie_inclusive.overlapped (frames from pinned host memory every step, copy under compute)'),
            note='`value` calls the same API on frames already resident in HBM, as the bench contract asks (six frame sets in '
                 'rotation); this is the figure with the frames arriving over PCIe as well')


def _variant_probes(args, est, dev, im_h, im_w, n_box, out):
    """The same step under other settings (72 depth bins, f16 autocast, backbone variants): N = 1, configs[1]."""
    if True:
        out['depth72'] = depth72_variant(args, dev, im_h, im_w, n_box)
        if args.precision == 'f32':
            out['f16_autocast'] = autocast_variant(args, dev, im_h, im_w, n_box)
        from metrabs_amd.models.metrabs import Metrabs
        if est.crop_model.backbone_is_pinned():
            # the product default pins MIOpen to its deterministic solvers for f32 arithmetic (Metrabs.
            # deterministic_backbone: replays and eager calls then agree bit for bit); the same step WITHOUT the pin
            before = Metrabs.deterministic_backbone
            Metrabs.deterministic_backbone = False
            try:
                out['backbone_not_pinned_deterministic'] = backbone_variant(
                    args, dev, im_h, im_w, n_box, not args.no_fold_bn, not args.no_fused_epilogue,
                    'same step as `value` with torch.backends.cudnn.deterministic left at PyTorch\'s default '
                    '(Metrabs.deterministic_backbone = False): MIOpen may pick atomically accumulating solvers -- the '
                    'same call can then differ run to run (features 7e-6 in f32, 7e-2 under f16 autocast on one box, '
                    '0.0 on another: profiles/r05f_ / r05z_backbone_determinism.jsonl)')
            finally:
                Metrabs.deterministic_backbone = before
        if not args.no_fold_bn:
            out['bn_not_folded'] = backbone_variant(
                args, dev, im_h, im_w, n_box, False, False,
                'same step as `value` with the backbone\'s batch norms as separate kernels and no '
                'K10 / K11 (--no-fold-bn): every backbone kernel is PyTorch-ROCm\'s own')
            if not args.no_fused_epilogue:
                out['bn_folded_torch_ops'] = backbone_variant(
                    args, dev, im_h, im_w, n_box, True, False,
                    'same step as `value` with the batch norms folded but bias / activation / skip / '
                    'mean and the depthwise layers left to PyTorch-ROCm\'s kernels (--no-fused-epilogue)')


if __name__ == '__main__':
    main()
