#!/usr/bin/env python
"""Per-shape A/B of the dense 3x3 convolutions of a 16-bit backbone copy at a bench shape (EfficientNetV2-S, batch 64,
256 px by default; --backbone effnetv2-l --batch 32 --res 384 is configs[4]; --backbone resnet18 works too):
K14h (kernels.conv3x3_bias_act16: one launch) against the path it replaces, the MIOpen convolution (unpinned, as
the 16-bit copy runs) followed by K10 (bias, activation, skip).

    python tools/conv3x3_ab.py --dtype f16 --out OUT.jsonl      # on the GPU

The method is tools/conv1x1_ab.py's: shape classes (Cin, Cout, H, W, stride, act, skip) are read from a hooked
forward of the folded copy; each arm is captured as a HIP graph of --iters calls and its replays are timed with
device events, the two arms alternated in --rounds rounds, the median per-call time reported with its share of
the 16-bit MFMA peak (2.5 PF) and of the byte floor (one 16-bit read of x, w and the skip, one write of y, at the
measured 6.29 TB/s copy rate of an MI355X).  Shapes the C entry declines are reported with k14h_us null.

    python tools/conv3x3_ab.py --dtype f32 --out OUT.jsonl      # K19 against what the f32 copy runs by default

--dtype f32: per shape class of the f32 copy folded with winograd3x3=True, K19 (kernels.conv3x3_winograd_bias_act)
against what the class runs in the default copy, by the same method.  A layer that stands alone (EfficientNetV2 stage
1, ResNet-18): the MIOpen convolution, pinned to the deterministic solvers as the f32 bench runs it, + K10.  The expand
of a FusedMBConv block (stages 2 - 3) is timed as the PAIR, because the prologue moves cost between the two kernels:
MIOpen convolution + K13 with the prologue against K19 + the plain K13 call.  Every record carries the per-round times
of both arms, the share of the 155 TF f32 matrix peak counted in Winograd-domain FLOP (16 products per 2x2 tile and
channel pair; the pair's project not counted) and the share of the byte floor of the 3x3 layer.
The stride-2 classes of the copy folded with strided3x3=True are timed in the same run, K22
(kernels.conv3x3_strided_bias_act) in the place of K19: a FusedMBConv expand as the pair (MIOpen pinned + K13 with the
prologue against K22 + the plain K13 call), a ResNet layer alone against MIOpen + K10; their records say stride 2 and
k22_*, and the share of the matrix peak is counted in direct-convolution FLOP.
The stride-1 classes with Cin % 8 == 0 get a THIRD arm in the same rounds, K21 (kernels.conv3x3_bias_act_split: the
f32 product on the bf16 matrix cores by operand split) in the place of K19 -- a layer as a layer, a FusedMBConv expand
as the pair K21 + the plain K13 call: k21_us, its rounds, whether it is ahead of the default arm and of K19 in every
round, and (a layer alone) the share of the 2.5 PF bf16 peak its six piece products reach.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK16_TF, PEAK32_TF, HBM_TBS = 2500.0, 155.0, 6.29


def shape_classes(res, backbone, dtype):
    import torch
    from metrabs_amd import backbones
    net = backbones.fold_batchnorm(backbones.build_backbone(backbone).eval(), fused_epilogue=True, dtype=dtype).cuda()
    out = {}
    for name, m in net.named_modules():
        if isinstance(m, backbones.Conv3x3BiasAct):
            def hook(mod, args, kwargs, name=name):
                x = args[0]
                key = (x.shape[1], mod.conv.out_channels, x.shape[2], x.shape[3], mod.stride, mod.act_name,
                       kwargs.get('residual') is not None)
                out.setdefault(key, []).append(name)
            m.register_forward_pre_hook(hook, with_kwargs=True)
    backbones.Conv3x3BiasAct.use_k14h = False
    with torch.inference_mode():
        net(torch.rand(1, 3, res, res, device='cuda'))
    backbones.Conv3x3BiasAct.use_k14h = True
    return out


def shape_classes_f32(res, backbone):
    """(Cin, Cout, H, W, act, skip, project Cout or None, stride) -> module names, from a hooked forward of the copy armed
    with winograd3x3 (the stride-1 classes, K19) and strided3x3 (the stride-2 classes, K22)."""
    import torch
    from metrabs_amd import backbones
    W3 = (backbones.WinogradConv3x3BiasAct, backbones.StridedConv3x3BiasAct)
    net = backbones.fold_batchnorm(backbones.build_backbone(backbone).eval(), fused_epilogue=True,
                                   winograd3x3=True, strided3x3=True).cuda()
    out, paired = {}, set()
    for name, m in net.named_modules():
        if isinstance(m, backbones.FusedMBConv) and m.pre_pair and isinstance(m.pre_pair[0], W3):
            paired.add(m.pre_pair[0])

            def hook(mod, args, name=name):
                x, (first, project) = args[0], mod.pre_pair
                key = (x.shape[1], first.conv.out_channels, x.shape[2], x.shape[3], first.act_name, mod.residual,
                       project.conv.out_channels, first.conv.stride[0])
                out.setdefault(key, []).append(name)
            m.register_forward_pre_hook(hook)
    for name, m in net.named_modules():
        if isinstance(m, W3) and m not in paired:
            def hook(mod, args, kwargs, name=name):
                x = args[0]
                key = (x.shape[1], mod.conv.out_channels, x.shape[2], x.shape[3], mod.act_name,
                       kwargs.get('residual') is not None, None, mod.conv.stride[0])
                out.setdefault(key, []).append(name)
            m.register_forward_pre_hook(hook, with_kwargs=True)
    W3[0].use_k19 = W3[1].use_k22 = False
    try:
        with torch.inference_mode():
            net(torch.rand(1, 3, res, res, device='cuda'))
    finally:
        W3[0].use_k19 = W3[1].use_k22 = True
    return out


def main_f32(args):
    import torch
    import torch.nn.functional as F
    from metrabs_amd import kernels
    classes = shape_classes_f32(args.res, args.backbone)
    rows = []
    g = torch.Generator(device='cuda').manual_seed(0)
    B = args.batch
    med = lambda v: sorted(v)[len(v) // 2]
    for (K, M, H, W, act, skip, P, stride), names in sorted(classes.items(), key=lambda kv: kv[1][0]):
        # tag: the kernel of the new arm, K19 for the stride-1 classes and K22 for the stride-2 ones
        tag, pack, takes, conv = {
            1: ('k19', kernels.pack_conv3x3_winograd_weight, kernels.conv3x3_winograd_supported,
                kernels.conv3x3_winograd_bias_act),
            2: ('k22', kernels.pack_conv3x3_strided_weight, kernels.conv3x3_strided_supported,
                kernels.conv3x3_strided_bias_act)}[stride]
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        x = torch.randn(B, K, H, W, device='cuda', generator=g)
        w = torch.randn(M, K, 3, 3, device='cuda', generator=g) / (9 * K) ** 0.5
        wu = pack(w)
        b = torch.randn(M, device='cuda', generator=g)
        y = torch.empty(B, M, Ho, Wo, device='cuda')
        supported = takes(x, wu)
        # the third arm of a stride-1 class: K21
        w21 = kernels.pack_conv3x3_split_weight(w) if stride == 1 and K % 8 == 0 else None
        third = w21 is not None and kernels.conv3x3_split_supported(x, w21)
        if P is None:
            r = torch.randn(B, M, Ho, Wo, device='cuda', generator=g) if skip else None

            def old():
                yy = F.conv2d(x, w, None, stride, 1)
                kernels.bias_act_(yy, b, act, r)
                return yy

            def new():
                return conv(x, wu, b, act, residual=r, out=y)

            def new21():
                return kernels.conv3x3_bias_act_split(x, w21, b, act, residual=r, out=y)
        else:
            w1 = torch.randn(P, M, 1, 1, device='cuda', generator=g) / M ** 0.5
            b1 = torch.randn(P, device='cuda', generator=g)
            r = torch.randn(B, P, Ho, Wo, device='cuda', generator=g) if skip else None

            def old():
                return kernels.conv1x1_bias_act(F.conv2d(x, w, None, stride, 1), w1, b1, None, residual=r, in_bias=b,
                                                in_act=act)

            def new():
                conv(x, wu, b, act, out=y)
                return kernels.conv1x1_bias_act(y, w1, b1, None, residual=r)

            def new21():
                kernels.conv3x3_bias_act_split(x, w21, b, act, out=y)
                return kernels.conv1x1_bias_act(y, w1, b1, None, residual=r)

        def captured(fn):
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                fn()
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    for _ in range(args.iters):
                        fn()
            torch.cuda.current_stream().wait_stream(st)
            torch.cuda.synchronize()
            return graph

        def timed(graph):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            graph.replay()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e3 / args.iters

        with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            a = old()
            diff = None
            if supported:
                c = new()
                torch.cuda.synchronize()
                diff = float((a - c).abs().max() / a.abs().max().clamp_min(1e-30))
            diff21 = None
            if third:
                c = new21()
                torch.cuda.synchronize()
                diff21 = float((a - c).abs().max() / a.abs().max().clamp_min(1e-30))
            for _ in range(3):
                old()
                if supported:
                    new()
                if third:
                    new21()
            arm_old = captured(old)
            arm_new = captured(new) if supported else None
            arm_21 = captured(new21) if third else None
            for _ in range(2):
                timed(arm_old)
                if supported:
                    timed(arm_new)
                if third:
                    timed(arm_21)
            t_old, t_new, t_21 = [], [], []
            for _ in range(args.rounds):
                t_old.append(timed(arm_old))
                if supported:
                    t_new.append(timed(arm_new))
                if third:
                    t_21.append(timed(arm_21))
            del arm_old, arm_new, arm_21
        direct_flop = 2.0 * B * Ho * Wo * 9 * K * M
        # what the new arm's MFMAs compute: the Winograd-domain products of K19, the direct convolution of K22
        wino_flop = 2.0 * B * (H // 2) * (W // 2) * 16 * K * M if stride == 1 else direct_flop
        byts = 4 * (B * (H * W * K + Ho * Wo * M * (2 if (skip and P is None) else 1)) + (16 if stride == 1 else 9) * M * K)
        byte_floor = byts / (HBM_TBS * 1e12) * 1e6
        row = dict(cin=K, cout=M, hw=f'{H}x{W}', stride=stride, act=act, skip=skip, project_cout=P,
                   timed='pair with the K13 project' if P is not None else 'layer', layers=len(names), first=names[0],
                   dtype='f32', batch=B, res=args.res, backbone=args.backbone,
                   direct_gflop=round(direct_flop / 1e9, 2), winograd_gflop=round(wino_flop / 1e9, 2) if stride == 1 else None,
                   mbytes=round(byts / 1e6, 1), old_us=round(med(t_old), 2), old_us_rounds=[round(t, 2) for t in t_old],
                   **{tag + '_us': None})
        if supported:
            t = med(t_new)
            row.update({tag + '_us': round(t, 2), tag + '_us_rounds': [round(v, 2) for v in t_new],
                        tag + '_ahead_in_every_round': max(t_new) < min(t_old)},
                       speedup=round(med(t_old) / t, 3), rel_diff=diff, byte_floor_us=round(byte_floor, 2))
            if P is None:   # (of a pair only the sum is timed: no share for the 3x3 layer alone)
                row.update({tag + ('_winograd_tflops' if stride == 1 else '_direct_tflops'): round(wino_flop / t / 1e6, 1),
                            tag + '_share_of_f32_peak': round(wino_flop / t / 1e6 / PEAK32_TF, 3)},
                           share_of_byte_floor=round(byte_floor / t, 3))
        if third:
            t = med(t_21)
            row.update(k21_us=round(t, 2), k21_us_rounds=[round(v, 2) for v in t_21],
                       k21_ahead_in_every_round=max(t_21) < min(t_old), k21_speedup=round(med(t_old) / t, 3),
                       k21_ahead_of_k19_in_every_round=bool(t_new) and max(t_21) < min(t_new), k21_rel_diff=diff21)
            if P is None:   # six bf16 piece products of the direct convolution
                row.update(k21_share_of_bf16_peak=round(6 * direct_flop / t / 1e6 / PEAK16_TF, 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--dtype', choices=['f16', 'bf16', 'f32'], default='f16')
    ap.add_argument('--backbone', default='effnetv2-s')
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.dtype == 'f32':
        return main_f32(args)
    import torch
    import torch.nn.functional as F
    from metrabs_amd import kernels
    dt = {'f16': torch.float16, 'bf16': torch.bfloat16}[args.dtype]
    classes = shape_classes(args.res, args.backbone, dt)
    rows = []
    g = torch.Generator(device='cuda').manual_seed(0)
    for (K, M, H, W, stride, act, res), names in sorted(classes.items(), key=lambda kv: kv[1][0]):
        B = args.batch
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        x = torch.randn(B, K, H, W, device='cuda', generator=g).to(dt)
        w = (torch.randn(M, K, 3, 3, device='cuda', generator=g) / (9 * K) ** 0.5).to(dt)
        wp = kernels.pack_conv3x3_weight(w)
        b = torch.randn(M, device='cuda', generator=g)
        r = torch.randn(B, M, Ho, Wo, device='cuda', generator=g).to(dt) if res else None
        y = torch.empty(B, M, Ho, Wo, device='cuda', dtype=dt)
        supported = kernels.conv3x3_16_supported(x, wp, stride)

        def old():
            yy = F.conv2d(x, w, None, stride, 1)
            kernels.bias_act_(yy, b, act, r)
            return yy

        def new():
            return kernels.conv3x3_bias_act16(x, wp, b, act, stride, residual=r, out=y)

        def captured(fn):
            """--iters calls of fn as one HIP graph (fn has run eagerly before: lazy set-up is done)."""
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                fn()
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    for _ in range(args.iters):
                        fn()
            torch.cuda.current_stream().wait_stream(st)
            torch.cuda.synchronize()
            return graph

        def timed(graph):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            graph.replay()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e3 / args.iters

        med = lambda v: sorted(v)[len(v) // 2]
        with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=False):
            a = old()
            diff = None
            if supported:
                c = new()
                torch.cuda.synchronize()
                diff = float((a - c).abs().max().float() / a.abs().max().float().clamp_min(1e-30))
            for _ in range(3):
                old()
                if supported:
                    new()
            arm_old = captured(old)
            arm_new = captured(new) if supported else None
            for _ in range(2):
                timed(arm_old)
                if supported:
                    timed(arm_new)
            t_old, t_new = [], []
            for _ in range(args.rounds):
                t_old.append(timed(arm_old))
                if supported:
                    t_new.append(timed(arm_new))
            del arm_old, arm_new
        flop = 2.0 * B * Ho * Wo * 9 * K * M
        byts = 2 * (B * (H * W * K + Ho * Wo * M * (2 if res else 1)) + 9 * M * K)
        byte_floor = byts / (HBM_TBS * 1e12) * 1e6
        row = dict(cin=K, cout=M, hw=f'{H}x{W}', stride=stride, act=act, skip=res, layers=len(names), first=names[0],
                   dtype=args.dtype, batch=B, res=args.res, backbone=args.backbone, gflop=round(flop / 1e9, 2),
                   mbytes=round(byts / 1e6, 1), old_us=round(med(t_old), 2),
                   old_tflops=round(flop / med(t_old) / 1e6, 1), k14h_us=None)
        if supported:
            t = med(t_new)
            row.update(k14h_us=round(t, 2), k14h_tflops=round(flop / t / 1e6, 1),
                       k14h_share_of_peak=round(flop / t / 1e6 / PEAK16_TF, 3), byte_floor_us=round(byte_floor, 2),
                       share_of_byte_floor=round(byte_floor / t, 3), speedup=round(med(t_old) / t, 3),
                       k14h_us_range=[round(min(t_new), 2), round(max(t_new), 2)],
                       old_us_range=[round(min(t_old), 2), round(max(t_old), 2)], rel_diff=diff)
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
