#!/usr/bin/env python
"""Per-shape A/B of the backbone stem at the bench shapes (EfficientNetV2-S batch 64 at 256 px, EfficientNetV2-L
batch 32 at 384 px, MobileNetV3 batch 320 at 256 px), for f32 / f16 / bf16 copies and planar / interleaved crops:
K17 (kernels.stem_conv_bias_act with preproc: one launch) against the chain it replaces as the default copy runs it,
Preproc (x * 2 - 1) + the MIOpen convolution + K10.  MIOpen runs unpinned for the 16-bit dtypes and under the
deterministic pin for f32, as those copies run.

    python tools/stem_ab.py --out OUT.jsonl      # on the GPU; everything in one call

The method is tools/conv3x3_ab.py's: each arm is captured as a HIP graph of --iters calls and its replays are timed
with device events, the two arms alternated in --rounds rounds, the median per-call time reported with the spread
of the rounds and K17's share of the byte floor (one read of the crops, one write of the activation, the weight, at
the measured 6.29 TB/s copy rate of an MI355X).  `ahead` says whether K17's slowest round beats the chain's fastest:
a shape where it does not belongs in backbones.StemConvBiasAct.k17_slower.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_TBS = 6.29
# (backbone, batch, res, Cout, activation)
SHAPES = [('effnetv2-s', 64, 256, 24, 'silu'), ('effnetv2-l', 32, 384, 32, 'silu'),
          ('mobilenetv3', 320, 256, 16, 'hardswish')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--dtypes', default='f16,bf16,f32')
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    from metrabs_amd import kernels
    dts = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}
    rows = []
    g = torch.Generator(device='cuda').manual_seed(0)
    for backbone, B, res, M, act in SHAPES:
        for dname in args.dtypes.split(','):
            dt = dts[dname]
            for layout in ('planar', 'interleaved'):
                x = torch.rand(B, 3, res, res, device='cuda', generator=g).to(dt)
                if layout == 'interleaved':
                    x = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
                w = (torch.randn(M, 3, 3, 3, device='cuda', generator=g) / 27 ** 0.5).to(dt)
                b = torch.randn(M, device='cuda', generator=g)
                y = torch.empty(B, M, res // 2, res // 2, device='cuda', dtype=dt)
                assert kernels.stem_conv_supported(x, w)

                def old():
                    yy = F.conv2d(x * 2 - 1, w, None, 2, 1)
                    if yy.is_contiguous():
                        kernels.bias_act_(yy, b, act)
                    else:   # a channels_last activation: K10 does not take it, the torch ops do
                        yy = getattr(F, act)(yy + b.view(1, -1, 1, 1).to(dt))
                    return yy

                def new():
                    return kernels.stem_conv_bias_act(x, w, b, act, preproc=True, out=y)

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
                with torch.inference_mode(), torch.backends.cudnn.flags(
                        enabled=True, benchmark=False, deterministic=dt == torch.float32):
                    a, c = old(), new()
                    torch.cuda.synchronize()
                    diff = float((a - c).abs().max().float() / a.abs().max().float().clamp_min(1e-30))
                    for _ in range(3):
                        old()
                        new()
                    arm_old, arm_new = captured(old), captured(new)
                    for _ in range(2):
                        timed(arm_old)
                        timed(arm_new)
                    t_old, t_new = [], []
                    for _ in range(args.rounds):
                        t_old.append(timed(arm_old))
                        t_new.append(timed(arm_new))
                    del arm_old, arm_new
                es = x.element_size()
                byts = es * (x.numel() + y.numel() + w.numel()) + 4 * M
                floor = byts / (HBM_TBS * 1e12) * 1e6
                row = dict(backbone=backbone, batch=B, res=res, cout=M, act=act, dtype=dname, layout=layout,
                           mbytes=round(byts / 1e6, 1), byte_floor_us=round(floor, 2),
                           chain_us=round(med(t_old), 2), k17_us=round(med(t_new), 2),
                           speedup=round(med(t_old) / med(t_new), 3), share_of_byte_floor=round(floor / med(t_new), 3),
                           chain_us_range=[round(min(t_old), 2), round(max(t_old), 2)],
                           k17_us_range=[round(min(t_new), 2), round(max(t_new), 2)],
                           ahead=bool(max(t_new) < min(t_old)), chain_out_nchw=bool(a.is_contiguous()), rel_diff=diff)
                rows.append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
