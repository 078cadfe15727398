#!/usr/bin/env python
"""Per-shape A/B of the 1x1 convolutions of EfficientNetV2-S at the bench shape (batch 64, 256 px, f32):
K13 (kernels.conv1x1_bias_act: one launch) against the path it replaces (x * gate where a squeeze-excite
block hands one over, the library convolution under the deterministic pin bench.py uses, K10).

    python tools/conv1x1_ab.py --out OUT.jsonl      # on the GPU

Shapes are read from a hooked forward of the folded network; each class (Cin, Cout, H, W, act, skip,
gate) is timed with device events over --iters calls per arm, the two arms alternated in rounds, and
reported as the median per-call time with its share of the 155 TF f32 MFMA peak and the HBM floor.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_TF, HBM_TBS = 155.0, 5.0


def shape_classes(batch, res):
    import torch
    from metrabs_amd import backbones
    net = backbones.fold_batchnorm(backbones.build_backbone('effnetv2-s').eval(), fused_epilogue=True).cuda()
    out = {}
    for name, m in net.named_modules():
        if isinstance(m, backbones.ConvBiasAct) and m.conv.kernel_size == (1, 1) and m.conv.stride == (1, 1):
            def hook(mod, args, kwargs, name=name):
                x = args[0]
                gated = any(mod in se.gate_to for se in net.modules() if isinstance(se, backbones.SqueezeExcite))
                key = (x.shape[1], mod.conv.out_channels, x.shape[2], x.shape[3], mod.act_name,
                       kwargs.get('residual') is not None, gated)
                out.setdefault(key, []).append(name)
            m.register_forward_pre_hook(hook, with_kwargs=True)
    backbones.ConvBiasAct.use_k13 = False
    with torch.inference_mode():
        net(torch.rand(1, 3, res, res, device='cuda'))
    backbones.ConvBiasAct.use_k13 = True
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    from metrabs_amd import kernels
    classes = shape_classes(args.batch, args.res)
    rows = []
    g = torch.Generator(device='cuda').manual_seed(0)
    for (K, M, H, W, act, res, gated), names in sorted(classes.items(), key=lambda kv: kv[1][0]):
        B = args.batch
        x = torch.randn(B, K, H, W, device='cuda', generator=g)
        w = torch.randn(M, K, 1, 1, device='cuda', generator=g) / K ** 0.5
        b = torch.randn(M, device='cuda', generator=g)
        gate = torch.rand(B, K, device='cuda', generator=g) if gated else None
        r = torch.randn(B, M, H, W, device='cuda', generator=g) if res else None
        y = torch.empty(B, M, H, W, device='cuda')

        def old():
            xi = x if gate is None else x * gate.view(B, K, 1, 1)
            yy = F.conv2d(xi, w)
            kernels.bias_act_(yy, b, act, r)
            return yy

        def new():
            return kernels.conv1x1_bias_act(x, w, b, act, gate=gate, residual=r, out=y)

        def timed(fn):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(args.iters):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e3 / args.iters

        with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            a, c = old(), new()
            torch.cuda.synchronize()
            diff = float((a - c).abs().max() / a.abs().max().clamp_min(1e-30))
            for _ in range(3):
                old(), new()
            t_old, t_new = [], []
            for _ in range(args.rounds):
                t_old.append(timed(old))
                t_new.append(timed(new))
        med = lambda v: sorted(v)[len(v) // 2]
        flop = 2.0 * B * H * W * K * M
        byts = 4.0 * (B * H * W * (K + M * (2 if res else 1)) + M * K)
        floor = max(flop / (PEAK_TF * 1e12), byts / (HBM_TBS * 1e12)) * 1e6
        row = dict(cin=K, cout=M, hw=f'{H}x{W}', act=act, skip=res, gate=gated, layers=len(names), first=names[0],
                   old_us=round(med(t_old), 2), k13_us=round(med(t_new), 2),
                   k13_tflops=round(flop / med(t_new) / 1e6, 1),
                   k13_share_of_peak=round(flop / med(t_new) / 1e6 / PEAK_TF, 3), floor_us=round(floor, 2),
                   speedup=round(med(t_old) / med(t_new), 3), rel_diff=diff)
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
