#!/usr/bin/env python
"""Whole-step A/B of the 16-bit backbone copy: bench.py's configs[1] (EfficientNetV2-S, 256 px, 64 crops) and
configs[4] (EfficientNetV2-L, 384 px, 32 crops, 122 joints) through Pose3dEstimator.estimate_poses_batched,
  A = the f32 folded copy under f16 autocast (bench.py's f16 mode, the reference's GPU arithmetic),
  B = the f16 folded copy (backbones.fold_batchnorm(dtype=torch.float16): K13h, weights cast once),
built from the same seeded network (bench.build_model), timed in interleaved pairs (A then B, --pairs times) with
device events over --steps calls each, reported as crops/s, plus each arm's MPJPE to the f32 folded model on the
same call (mm).  Both arms run with the estimator's API graphs as a user gets them (graph_batches 'auto': each
internal batch shape is captured on its second call and replayed after; --graph-batches off for eager calls);
the graph cache's replay counts are reported with each pair.  bench.py itself is only imported.
--ab k14h compares the 16-bit copy with itself instead: A = Conv3x3BiasAct.use_k14h off (the dense 3x3 layers on MIOpen
+ K10), B = on (K14h); the same tree and weights, so the pairs isolate K14h.  The rows keep their field names
(autocast_* = arm A, copy_* = arm B) and carry ab='k14h'.
--ab k15 does the same for the depthwise 5x5 layers (MobileNetV3: --config 3, 64 boxes x 5 augmentations): both arms
are folded from the same network, A with DepthwiseBiasAct.kernel_sizes = (3,) at fold time (the 5x5 layers as
DepthwiseConv2d + K10, the tree from before K15), B with (3, 5) (K15); --dtype f32 compares the f32 copies, f16 /
bf16 the 16-bit copies.  The rows carry ab='k15'.
--ab k16h: both arms are the 16-bit copy of the same network, A folded as by default, B with fuse_blocks=True (its
FusedMBConv blocks of stages 2 - 3 as one launch each, K16h, where FusedMBConv.k16h_slower does not list them).  The
rows carry ab='k16h'.
--ab k17: both arms are the same copy of the same network (16-bit, or f32 with --dtype f32; --config 1, 3 or 4), A
folded as by default, B with fuse_stem=True (Preproc + the stem convolution + its epilogue as one launch, K17).  The
rows carry ab='k17'.
--ab k18: both arms are the same copy of the same network (16-bit, or f32 with --dtype f32; --config 3 or 4), A folded
as by default, B with block_depthwise=True (the stride-1 depthwise 3x3 layers on K18 where K11 would take its generic
kernel).  The arms return the same poses bit for bit.  The rows carry ab='k18'.
--ab deepk: both arms are the 16-bit copy of the same network (--config 1 or 4), A folded as by default, B with
deep_projects=True (the deep project convolutions on K13h's deep-K configuration instead of cast + x * gate + rocBLAS +
K10).  The arms differ by rounding; the rows carry ab='deepk' and the paths of the armed layers.
--ab k19: both arms are the f32 copy of the same network (--dtype f32; --config 1), A folded as by default, B with
winograd3x3=True (the dense 3x3 stride-1 layers on K19 where WinogradConv3x3BiasAct.k19_slower does not list them).  The
arms differ by rounding; the rows carry ab='k19' and the paths of the armed layers.
--ab k20: both arms are the f32 copy of the same network (--dtype f32; --config 1, 3 or 4), A folded as by default, B with
split_gemm=True (the 1x1 stride-1 layers on K20, the split-operand kernel, where ConvBiasAct.k20_slower does not list
them); --winograd3x3 folds BOTH arms with winograd3x3=True as well.  The arms differ by rounding; the rows carry
ab='k20' and the paths of the 1x1 layers of both arms.
--ab k22: both arms are the f32 copy of the same network (--dtype f32; --config 1), A folded as by default, B with
strided3x3=True (the dense 3x3 stride-2 layers on K22 where StridedConv3x3BiasAct.k22_slower does not list them);
--winograd3x3 folds BOTH arms with winograd3x3=True as well.  The arms differ by rounding; the rows carry ab='k22', the
paths of the armed layers and the MPJPE between the two arms' poses.
--ab k21: both arms are the f32 copy of the same network (--dtype f32; --config 1), A folded as by default, B with
split3x3=True (the dense 3x3 stride-1 layers on K21 where SplitConv3x3BiasAct.k21_slower does not list them);
--winograd3x3 folds BOTH arms with winograd3x3=True as well (B then runs K19 where K21 leaves a layer).  The arms differ
by rounding; the rows carry ab='k21', the paths of the armed layers and the MPJPE between the two arms' poses.
--ab k27h: both arms are the 16-bit copy of the same network (--config 3, MobileNetV3), A folded as by default, B with
fuse_expand_depthwise_tiles=True (the expand + depthwise 3x3 pairs on large planes as one launch, K27h, where
DepthwiseBiasAct.k27h_slower does not list them).  The rows carry ab='k27h' and the paths of the armed expands.
--ab k28h: the same with fuse_expand_depthwise5x5=True (the expand + depthwise 5x5 pairs as one launch, K28h, where
DepthwiseBiasAct.k28h_slower does not list them).  The rows carry ab='k28h' and the paths of the armed expands.

    python tools/backbone16_ab.py --config 1 --out OUT.jsonl      # on the GPU
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', type=int, default=1, choices=[1, 3, 4])
    ap.add_argument('--pairs', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dtype', choices=['f16', 'bf16', 'f32'], default='f16')
    ap.add_argument('--graph-batches', choices=['auto', 'off'], default='auto')
    ap.add_argument('--ab', choices=['copy', 'k14h', 'k15', 'k16h', 'k17', 'k18', 'deepk', 'k19', 'k20', 'k21', 'k22',
                                     'k25h', 'k26h', 'k27h', 'k28h'],
                    default='copy',
                    help="copy: autocast vs the 16-bit copy; k14h: the copy with K14h off vs on; k15: the copy (f32 with "
                         "--dtype f32) folded without vs with K15; k16h: the copy folded without vs with fuse_blocks; k17: without vs with fuse_stem; "
                         "k18: without vs with block_depthwise; deepk: without vs with deep_projects; "
                         "k19 (--dtype f32): the f32 copy folded without vs with winograd3x3; "
                         "k20 (--dtype f32): the f32 copy folded without vs with split_gemm; "
                         "k21 (--dtype f32): the f32 copy folded without vs with split3x3; "
                         "k22 (--dtype f32): the f32 copy folded without vs with strided3x3; "
                         "k25h: the 16-bit copy folded without vs with fuse_expand_depthwise; "
                         "k26h: the 16-bit copy folded without vs with fuse_expand_depthwise_planes (--config 4, or "
                         "--config 1 --res 384); "
                         "k27h: the 16-bit copy folded without vs with fuse_expand_depthwise_tiles (--config 3); "
                         "k28h: the 16-bit copy folded without vs with fuse_expand_depthwise5x5 (--config 3)")
    ap.add_argument('--res', type=int, default=None, help='crop side handed to bench.py (its --res) instead of the '
                                                          "config's own")
    ap.add_argument('--winograd3x3', action='store_true',
                    help='--ab k20, --ab k21, --ab k22: fold both arms with winograd3x3=True too')
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    if (args.dtype == 'f32' or args.config == 3) and args.ab not in ('k15', 'k17', 'k18', 'k19', 'k20', 'k21', 'k22') \
            and not (args.ab in ('k27h', 'k28h') and args.dtype != 'f32'):
        ap.error('--dtype f32 and --config 3 go with --ab k15, --ab k17, --ab k18, --ab k19, --ab k20, --ab k21 or --ab k22 '
                 '(--config 3 with a 16-bit dtype also with --ab k27h and --ab k28h)')
    if args.ab in ('k19', 'k20', 'k21', 'k22') and args.dtype != 'f32':
        ap.error(f'--ab {args.ab} goes with --dtype f32')
    if args.winograd3x3 and args.ab not in ('k20', 'k21', 'k22'):
        ap.error('--winograd3x3 goes with --ab k20, --ab k21 or --ab k22')
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    from metrabs_amd.backbones import Conv3x3BiasAct, ConvBiasAct, DepthwiseBiasAct, fold_batchnorm
    dt = {'f16': torch.float16, 'bf16': torch.bfloat16, 'f32': None}[args.dtype]
    argv, sys.argv = sys.argv, ['bench.py', '--config', str(args.config), '--precision', args.dtype] \
        + ([] if args.res is None else ['--res', str(args.res)])
    bargs = bench.parse_args()
    sys.argv = argv
    dev = torch.device('cuda')
    est_a, _ = bench.build_model(bargs, dev)                     # f32 copy under 16-bit autocast
    est_b, _ = bench.build_model(bargs, dev)                     # the same seeded network ...
    if dt is not None:
        est_b.crop_model.backbone = fold_batchnorm(est_b.reference_backbone, fused_epilogue=True, dtype=dt)
        est_b.crop_dtype = est_b.crop_model.input_dtype          # ... as its 16-bit copy
    if args.ab == 'k16h':                                        # both arms the 16-bit copy, B with its blocks armed
        from metrabs_amd.backbones import FusedMBConv
        est_a.crop_model.backbone = fold_batchnorm(est_a.reference_backbone, fused_epilogue=True, dtype=dt)
        est_a.crop_dtype = est_a.crop_model.input_dtype
        est_b.crop_model.backbone = fold_batchnorm(est_b.reference_backbone, fused_epilogue=True, dtype=dt,
                                                   fuse_blocks=True)
        assert any(isinstance(m, FusedMBConv) and m.fused_pair for m in est_b.crop_model.backbone.modules())
    if args.ab == 'k17':                                         # both arms the same copy, B with its stem on K17
        from metrabs_amd.backbones import StemConvBiasAct
        est_a.crop_model.backbone = fold_batchnorm(est_a.reference_backbone, fused_epilogue=True, dtype=dt)
        est_b.crop_model.backbone = fold_batchnorm(est_b.reference_backbone, fused_epilogue=True, dtype=dt,
                                                   fuse_stem=True)
        for e in (est_a, est_b):
            e.crop_dtype = e.crop_model.input_dtype
            if dt is None:
                e.crop_model.autocast_dtype = None               # f32 copies, run in f32
        assert any(isinstance(m, StemConvBiasAct) for m in est_b.crop_model.backbone.modules())
    if args.ab == 'k18':                                         # both arms the same copy, B with K18 armed
        est_a.crop_model.backbone = fold_batchnorm(est_a.reference_backbone, fused_epilogue=True, dtype=dt)
        est_b.crop_model.backbone = fold_batchnorm(est_b.reference_backbone, fused_epilogue=True, dtype=dt,
                                                   block_depthwise=True)
        for e in (est_a, est_b):
            e.crop_dtype = e.crop_model.input_dtype
            if dt is None:
                e.crop_model.autocast_dtype = None               # f32 copies, run in f32
        assert any(isinstance(m, DepthwiseBiasAct) and m.block_depthwise for m in est_b.crop_model.backbone.modules())
    if args.ab == 'k19':                                         # both arms the f32 copy, B with K19 armed
        from metrabs_amd.backbones import WinogradConv3x3BiasAct
        est_a.crop_model.backbone = fold_batchnorm(est_a.reference_backbone, fused_epilogue=True)
        est_b.crop_model.backbone = fold_batchnorm(est_b.reference_backbone, fused_epilogue=True, winograd3x3=True)
        for e in (est_a, est_b):
            e.crop_dtype = e.crop_model.input_dtype
            e.crop_model.autocast_dtype = None                   # f32 copies, run in f32
        assert any(isinstance(m, WinogradConv3x3BiasAct) for m in est_b.crop_model.backbone.modules())
    if args.ab == 'k20':                                         # both arms the f32 copy, B with K20 armed
        est_a.crop_model.backbone = fold_batchnorm(est_a.reference_backbone, fused_epilogue=True,
                                                   winograd3x3=args.winograd3x3)
        est_b.crop_model.backbone = fold_batchnorm(est_b.reference_backbone, fused_epilogue=True,
                                                   winograd3x3=args.winograd3x3, split_gemm=True)
        for e in (est_a, est_b):
            e.crop_dtype = e.crop_model.input_dtype
            e.crop_model.autocast_dtype = None                   # f32 copies, run in f32
        assert any(isinstance(m, ConvBiasAct) and m.split_gemm for m in est_b.crop_model.backbone.modules())
    if args.ab == 'k21':                                         # both arms the f32 copy, B with K21 armed
        from metrabs_amd.backbones import SplitConv3x3BiasAct
        est_a.crop_model.backbone = fold_batchnorm(est_a.reference_backbone, fused_epilogue=True,
                                                   winograd3x3=args.winograd3x3)
        est_b.crop_model.backbone = fold_batchnorm(est_b.reference_backbone, fused_epilogue=True,
                                                   winograd3x3=args.winograd3x3, split3x3=True)
        for e in (est_a, est_b):
            e.crop_dtype = e.crop_model.input_dtype
            e.crop_model.autocast_dtype = None                   # f32 copies, run in f32
        assert any(isinstance(m, SplitConv3x3BiasAct) for m in est_b.crop_model.backbone.modules())
    if args.ab == 'k22':                                         # both arms the f32 copy, B with K22 armed
        from metrabs_amd.backbones import StridedConv3x3BiasAct
        est_a.crop_model.backbone = fold_batchnorm(est_a.reference_backbone, fused_epilogue=True,
                                                   winograd3x3=args.winograd3x3)
        est_b.crop_model.backbone = fold_batchnorm(est_b.reference_backbone, fused_epilogue=True,
                                                   winograd3x3=args.winograd3x3, strided3x3=True)
        for e in (est_a, est_b):
            e.crop_dtype = e.crop_model.input_dtype
            e.crop_model.autocast_dtype = None                   # f32 copies, run in f32
        assert any(isinstance(m, StridedConv3x3BiasAct) for m in est_b.crop_model.backbone.modules())
    if args.ab == 'deepk':                                       # both arms the 16-bit copy, B with its deep projects armed
        est_a.crop_model.backbone = fold_batchnorm(est_a.reference_backbone, fused_epilogue=True, dtype=dt)
        est_a.crop_dtype = est_a.crop_model.input_dtype
        est_b.crop_model.backbone = fold_batchnorm(est_b.reference_backbone, fused_epilogue=True, dtype=dt,
                                                   deep_projects=True)
        assert any(isinstance(m, ConvBiasAct) and m.deep_projects for m in est_b.crop_model.backbone.modules())
    if args.ab == 'k25h':                                        # both arms the 16-bit copy, B with its MBConv pairs armed
        est_a.crop_model.backbone = fold_batchnorm(est_a.reference_backbone, fused_epilogue=True, dtype=dt)
        est_a.crop_dtype = est_a.crop_model.input_dtype
        est_b.crop_model.backbone = fold_batchnorm(est_b.reference_backbone, fused_epilogue=True, dtype=dt,
                                                   fuse_expand_depthwise=True)
        assert any(isinstance(m, ConvBiasAct) and m.hand_to for m in est_b.crop_model.backbone.modules())
    if args.ab == 'k26h':                                        # the same, armed for the planes of a 384 px input
        est_a.crop_model.backbone = fold_batchnorm(est_a.reference_backbone, fused_epilogue=True, dtype=dt)
        est_a.crop_dtype = est_a.crop_model.input_dtype
        est_b.crop_model.backbone = fold_batchnorm(est_b.reference_backbone, fused_epilogue=True, dtype=dt,
                                                   fuse_expand_depthwise_planes=True)
        assert any(isinstance(m, ConvBiasAct) and m.hand_planes_to for m in est_b.crop_model.backbone.modules())
    if args.ab == 'k27h':                                        # the same, armed for MobileNetV3's large planes
        est_a.crop_model.backbone = fold_batchnorm(est_a.reference_backbone, fused_epilogue=True, dtype=dt)
        est_a.crop_dtype = est_a.crop_model.input_dtype
        est_b.crop_model.backbone = fold_batchnorm(est_b.reference_backbone, fused_epilogue=True, dtype=dt,
                                                   fuse_expand_depthwise_tiles=True)
        assert any(isinstance(m, ConvBiasAct) and m.hand_tiles_to for m in est_b.crop_model.backbone.modules())
    if args.ab == 'k28h':                                        # the same, armed for MobileNetV3's 5x5 pairs
        est_a.crop_model.backbone = fold_batchnorm(est_a.reference_backbone, fused_epilogue=True, dtype=dt)
        est_a.crop_dtype = est_a.crop_model.input_dtype
        est_b.crop_model.backbone = fold_batchnorm(est_b.reference_backbone, fused_epilogue=True, dtype=dt,
                                                   fuse_expand_depthwise5x5=True)
        assert any(isinstance(m, ConvBiasAct) and m.hand_k5_to for m in est_b.crop_model.backbone.modules())
    if args.ab == 'k14h':                                        # arm A: the same copy, K14h switched off
        est_a.crop_model.backbone = fold_batchnorm(est_a.reference_backbone, fused_epilogue=True, dtype=dt)
        est_a.crop_dtype = est_a.crop_model.input_dtype
    if args.ab == 'k15':                                         # arm A: the same copy, folded as before K15
        DepthwiseBiasAct.kernel_sizes = (3,)
        est_a.crop_model.backbone = fold_batchnorm(est_a.reference_backbone, fused_epilogue=True, dtype=dt)
        DepthwiseBiasAct.kernel_sizes = (3, 5)
        est_a.crop_dtype = est_a.crop_model.input_dtype
        assert not any(isinstance(m, DepthwiseBiasAct) and m.k == 5 for m in est_a.crop_model.backbone.modules())
        assert any(isinstance(m, DepthwiseBiasAct) and m.k == 5 for m in est_b.crop_model.backbone.modules())
    est_f, _ = bench.build_model(bargs, dev)                     # f32 folded: the accuracy reference
    est_f.crop_model.autocast_dtype = None
    est_f.crop_dtype = torch.float32
    for e in (est_a, est_b):
        e.graph_batches = 'auto' if args.graph_batches == 'auto' else False
    est_f.graph_batches = False

    g = torch.Generator().manual_seed(5)
    n_box, frames, im_h, im_w = bargs.batch // max(bargs.num_aug, 1), bargs.frames, 1080, 1920   # (boxes, each sampled num_aug times)
    images = torch.randint(0, 256, (frames, 3, im_h, im_w), dtype=torch.uint8, generator=g).to(dev)
    bw = 60 + 340 * torch.rand(n_box, generator=g)
    bh = 150 + 750 * torch.rand(n_box, generator=g)
    bx = torch.rand(n_box, generator=g) * (im_w - bw)
    by = torch.rand(n_box, generator=g) * (im_h - bh).clamp_min(1.0)
    allb = torch.stack([bx, by, bw, bh], dim=1)
    ids = (torch.arange(n_box) * frames) // n_box
    boxes = [allb[ids == i] for i in range(frames)]
    f = max(im_h, im_w) / (np.tan(np.deg2rad(55.0) / 2) * 2)
    K = torch.tensor([[f, 0, im_w / 2], [0, f, im_h / 2], [0, 0, 1]], dtype=torch.float32).repeat(frames, 1, 1)

    def call(est):
        # the class switch is read when a forward runs eagerly or is captured; a replayed graph keeps its arm
        Conv3x3BiasAct.use_k14h = not (args.ab == 'k14h' and est is est_a)
        r = est.estimate_poses_batched(images, boxes, intrinsic_matrix=K, internal_batch_size=bargs.batch,
                                       num_aug=bargs.num_aug)
        return torch.cat(r['poses3d'])

    def timed(est):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(args.steps):
            call(est)
        ev[1].record()
        torch.cuda.synchronize()
        return bargs.batch * args.steps / (ev[0].elapsed_time(ev[1]) / 1e3)

    rows = []
    with torch.inference_mode():
        p_f, p_a, p_b = call(est_f), call(est_a), call(est_b)
        mpjpe = lambda p: float((p - p_f).norm(dim=-1).mean())
        acc = dict(kind='accuracy', config=args.config, dtype=args.dtype, mpjpe_autocast_mm=round(mpjpe(p_a), 4),
                   mpjpe_copy_mm=round(mpjpe(p_b), 4))
        print(json.dumps(acc), flush=True)
        rows.append(acc)
        for _ in range(args.warmup):
            call(est_a), call(est_b)
        torch.cuda.synchronize()
        for i in range(args.pairs):
            a, b = timed(est_a), timed(est_b)
            row = dict(kind='pair', ab=args.ab, config=args.config, dtype=args.dtype, graph_batches=args.graph_batches, pair=i,
                       autocast_crops_per_s=round(a, 1), copy_crops_per_s=round(b, 1), gain=round(b / a - 1, 4),
                       autocast_graph_replays=est_a.graphs.stats['replays'],
                       copy_graph_replays=est_b.graphs.stats['replays'])
            print(json.dumps(row), flush=True)
            rows.append(row)
    if args.ab == 'k16h':
        from metrabs_amd.backbones import FusedMBConv
        paths = [m.last_path for m in est_b.crop_model.backbone.modules()
                 if isinstance(m, FusedMBConv) and m.fused_pair]
        row = dict(kind='paths', ab='k16h', k16h=paths.count('k16h'), chain=paths.count('chain'))
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.ab == 'k25h':
        paths = [m.last_path for m in est_b.crop_model.backbone.modules() if isinstance(m, ConvBiasAct) and m.hand_to]
        row = dict(kind='paths', ab='k25h', equal_poses=bool(torch.equal(p_a, p_b)),
                   b={str(k): paths.count(k) for k in sorted(set(paths), key=str)})
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.ab == 'k26h':
        paths = [m.last_path for m in est_b.crop_model.backbone.modules()
                 if isinstance(m, ConvBiasAct) and m.hand_planes_to]
        row = dict(kind='paths', ab='k26h', res=bargs.res, backbone=bargs.backbone, batch=bargs.batch,
                   equal_poses=bool(torch.equal(p_a, p_b)),
                   b={str(k): paths.count(k) for k in sorted(set(paths), key=str)})
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.ab == 'k27h':
        paths = [m.last_path for m in est_b.crop_model.backbone.modules()
                 if isinstance(m, ConvBiasAct) and m.hand_tiles_to]
        row = dict(kind='paths', ab='k27h', res=bargs.res, backbone=bargs.backbone, batch=bargs.batch,
                   equal_poses=bool(torch.equal(p_a, p_b)),
                   b={str(k): paths.count(k) for k in sorted(set(paths), key=str)})
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.ab == 'k28h':
        paths = [m.last_path for m in est_b.crop_model.backbone.modules()
                 if isinstance(m, ConvBiasAct) and m.hand_k5_to]
        row = dict(kind='paths', ab='k28h', res=bargs.res, backbone=bargs.backbone, batch=bargs.batch,
                   equal_poses=bool(torch.equal(p_a, p_b)),
                   b={str(k): paths.count(k) for k in sorted(set(paths), key=str)})
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.ab == 'k17':
        from metrabs_amd.backbones import StemConvBiasAct
        row = dict(kind='paths', ab='k17', stem=[m.last_path for m in est_b.crop_model.backbone.modules()
                                                  if isinstance(m, StemConvBiasAct)])
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.ab == 'k18':
        paths = [[m.last_path for m in e.crop_model.backbone.modules() if isinstance(m, DepthwiseBiasAct) and m.k == 3]
                 for e in (est_a, est_b)]
        row = dict(kind='paths', ab='k18', equal_poses=bool(torch.equal(p_a, p_b)),
                   a={k: paths[0].count(k) for k in sorted(set(paths[0]))},
                   b={k: paths[1].count(k) for k in sorted(set(paths[1]))})
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.ab == 'k19':
        from metrabs_amd.backbones import WinogradConv3x3BiasAct
        paths = [m.last_path for m in est_b.crop_model.backbone.modules() if isinstance(m, WinogradConv3x3BiasAct)]
        row = dict(kind='paths', ab='k19', mpjpe_armed_vs_default_mm=round(float((p_b - p_a).norm(dim=-1).mean()), 5),
                   b={k: paths.count(k) for k in sorted(set(paths))})
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.ab == 'k20':
        paths = [[m.last_path for m in e.crop_model.backbone.modules() if isinstance(m, ConvBiasAct)
                  and m.conv.kernel_size == (1, 1)] for e in (est_a, est_b)]
        row = dict(kind='paths', ab='k20', winograd3x3=args.winograd3x3,
                   mpjpe_armed_vs_default_mm=round(float((p_b - p_a).norm(dim=-1).mean()), 5),
                   a={str(k): paths[0].count(k) for k in sorted(set(paths[0]), key=str)},
                   b={str(k): paths[1].count(k) for k in sorted(set(paths[1]), key=str)})
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.ab == 'k21':
        from metrabs_amd.backbones import SplitConv3x3BiasAct
        paths = [m.last_path for m in est_b.crop_model.backbone.modules() if isinstance(m, SplitConv3x3BiasAct)]
        row = dict(kind='paths', ab='k21', winograd3x3=args.winograd3x3,
                   mpjpe_armed_vs_default_mm=round(float((p_b - p_a).norm(dim=-1).mean()), 5),
                   b={str(k): paths.count(k) for k in sorted(set(paths), key=str)})
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.ab == 'k22':
        from metrabs_amd.backbones import StridedConv3x3BiasAct
        paths = [m.last_path for m in est_b.crop_model.backbone.modules() if isinstance(m, StridedConv3x3BiasAct)]
        row = dict(kind='paths', ab='k22', winograd3x3=args.winograd3x3,
                   mpjpe_armed_vs_default_mm=round(float((p_b - p_a).norm(dim=-1).mean()), 5),
                   b={str(k): paths.count(k) for k in sorted(set(paths), key=str)})
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.ab == 'deepk':
        paths = [[m.last_path for m in e.crop_model.backbone.modules() if isinstance(m, ConvBiasAct)
                  and (m.act is None and m.conv.in_channels >= 768 and m.conv.out_channels > 160
                       and m.conv.kernel_size == (1, 1))] for e in (est_a, est_b)]
        row = dict(kind='paths', ab='deepk', a={k: paths[0].count(k) for k in sorted(set(paths[0]))},
                   b={k: paths[1].count(k) for k in sorted(set(paths[1]))})
        print(json.dumps(row), flush=True)
        rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        for r in rows:
            fh.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
