#!/usr/bin/env python
"""Per-shape A/B of the depthwise 5x5 layers of a folded backbone (MobileNetV3-Large, batch 320, 256 px by default =
configs[3]): K15 (kernels.depthwise5x5_bias_act: one launch, plane mean included) against the path it replaces,
PyTorch's depthwise kernel (backbones.DepthwiseConv2d, MIOpen off for it) followed by K10 with the plane mean
(kernels.bias_act_rowmean_) -- in a 16-bit run with the 16-bit weight the copy used to hold.

    python tools/depthwise_ab.py --dtype f32 --out OUT.jsonl      # on the GPU

The method is tools/conv3x3_ab.py's, with one difference: the kernel is HBM-bound, so every arm works on a ring of
input buffers that together exceed --ring-mib (256 MiB, the size of the last-level cache) -- one call per buffer,
the whole ring captured as one HIP graph; a cache-hot timing would flatter both arms, K15 more.  The arms are
alternated in --rounds rounds; reported are the median per-call time, its range, the speed-up and the share of the
byte floor (activation in + out + the means, at the measured 6.29 TB/s copy rate of an MI355X).  `verdict` is
'k15' only if K15's median is below the old path's by more than K15's own round-to-round range, else
'k15_slower': the (C, H, W, stride) to enter into backbones.DepthwiseBiasAct.k15_slower.

    python tools/depthwise_ab.py --arm k18 --dtype f16 --shapes 768x24x24,1344x24x24 --batch 32 --out OUT.jsonl

--arm k18: K11 (kernels.depthwise3x3_bias_act) against K18 (kernels.depthwise3x3_blocks_bias_act), stride 1 and
padding 1, with the plane mean, on the (C x H x W) classes of --shapes (default: the classes of EfficientNetV2-L at
384 px and MobileNetV3 at 256 px that K11 runs on its generic kernel), the same ring and rounds.  In 16 bits both of
K18's block shapes (4 and 8 columns per lane, the latter where W % 8 == 0) are timed.  A class -- and a block shape
-- stays on K18 only if it is faster than the other arm in EVERY round, else the verdict is 'k18_slower': the
(C, H, W) to enter into backbones.DepthwiseBiasAct.k18_slower.  The outputs and means of the arms must be equal bit
for bit where K11 takes its generic kernel ('equal' in the row); on the planes K11's block kernel takes (960x16x16
with K18 forced, for comparison) they are two roundings apart.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_TBS = 6.29


def shape_classes(res, backbone):
    import torch
    from metrabs_amd import backbones
    net = backbones.fold_batchnorm(backbones.build_backbone(backbone).eval(), fused_epilogue=True).cuda()
    out = {}
    for name, m in net.named_modules():
        if isinstance(m, backbones.DepthwiseBiasAct) and m.k == 5:
            def hook(mod, args, name=name):
                x = args[0]
                pad = mod.pad if mod.pads is None else tuple(mod.pads)
                out.setdefault((x.shape[1], x.shape[2], x.shape[3], mod.stride, pad, mod.act_name, mod.emit_mean),
                               []).append(name)
            m.register_forward_pre_hook(hook)
    with torch.inference_mode():
        net(torch.rand(1, 3, res, res, device='cuda'))
    return out


K18_SHAPES = '768x24x24,1344x24x24,2304x12x12,3840x12x12,16x128x128,72x64x64'


def main_k18(args):
    import torch
    from metrabs_amd import kernels
    dt = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}[args.dtype]
    es = 4 if dt == torch.float32 else 2
    g = torch.Generator(device='cuda').manual_seed(0)
    rows = []
    for spec in (args.shapes or K18_SHAPES).split(','):
        C, H, W = (int(v) for v in spec.split('x'))
        B = args.batch
        byts = B * C * 2 * H * W * es + B * C * 4
        n_ring = max(2, -(-args.ring_mib * 2 ** 20 // byts) + 1)
        xs = [torch.randn(B, C, H, W, device='cuda', generator=g).to(dt) for _ in range(n_ring)]
        w = torch.randn(C, 1, 3, 3, device='cuda', generator=g) * 0.4
        b = torch.randn(C, device='cuda', generator=g)
        arms = {'k11': lambda x: kernels.depthwise3x3_bias_act(x, w, b, args.act, 1, 1, want_mean=True),
                'k18_4': lambda x: kernels.depthwise3x3_blocks_bias_act(x, w, b, args.act, want_mean=True, block_cols=4)}
        if es == 2 and W % 8 == 0:
            arms['k18_8'] = lambda x: kernels.depthwise3x3_blocks_bias_act(x, w, b, args.act, want_mean=True,
                                                                           block_cols=8)

        def captured(fn):
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                fn(xs[0])
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    for x in xs:
                        fn(x)
            torch.cuda.current_stream().wait_stream(st)
            torch.cuda.synchronize()
            return graph

        def timed(graph):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            graph.replay()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e3 / n_ring

        med = lambda v: sorted(v)[len(v) // 2]
        with torch.inference_mode():
            outs = {k: fn(xs[0]) for k, fn in arms.items()}
            torch.cuda.synchronize()
            equal = all(torch.equal(outs['k11'][0], o[0]) and torch.equal(outs['k11'][1], o[1]) for o in outs.values())
            del outs
            graphs = {k: captured(fn) for k, fn in arms.items()}
            for _ in range(2):
                for gr in graphs.values():
                    timed(gr)
            t = {k: [] for k in arms}
            for _ in range(args.rounds):
                for k, gr in graphs.items():
                    t[k].append(timed(gr))
            del graphs
        floor = byts / (HBM_TBS * 1e12) * 1e6
        every = lambda a, c: all(x < y for x, y in zip(t[a], t[c]))   # a faster than c in every round
        shape = 'k18_4'
        if 'k18_8' in t and every('k18_8', 'k18_4'):
            shape = 'k18_8'
        row = dict(c=C, hw=f'{H}x{W}', act=args.act, dtype=args.dtype, batch=B, ring=n_ring,
                   mbytes=round(byts / 1e6, 1), byte_floor_us=round(floor, 2), equal_bits=equal,
                   k11_takes_block_kernel=kernels.k11_takes_block_kernel(H, W))
        for k in t:
            row[k + '_us'] = round(med(t[k]), 2)
            row[k + '_us_range'] = [round(min(t[k]), 2), round(max(t[k]), 2)]
            row[k + '_share_of_byte_floor'] = round(floor / med(t[k]), 3)
        row.update(block_cols=int(shape[4:]), speedup=round(med(t['k11']) / med(t[shape]), 3),
                   verdict='k18' if every(shape, 'k11') else 'k18_slower', key=[C, H, W])
        rows.append(row)
        print(json.dumps(row), flush=True)
        del xs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--arm', choices=['k15', 'k18'], default='k15')
    ap.add_argument('--shapes', default=None, help='--arm k18: comma-separated CxHxW classes')
    ap.add_argument('--act', default='silu', help='--arm k18: the activation (none: pass "")')
    ap.add_argument('--batch', type=int, default=320)
    ap.add_argument('--res', type=int, default=256)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--ring-mib', type=int, default=256)
    ap.add_argument('--dtype', choices=['f32', 'f16', 'bf16'], default='f32')
    ap.add_argument('--backbone', default='mobilenetv3')
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    if args.arm == 'k18':
        args.act = args.act or None
        return main_k18(args)
    import torch
    import torch.nn.functional as F
    from metrabs_amd import backbones, kernels
    dt = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}[args.dtype]
    classes = shape_classes(args.res, args.backbone)
    rows = []
    g = torch.Generator(device='cuda').manual_seed(0)
    for (C, H, W, stride, pad, act, want_mean), names in sorted(classes.items(), key=lambda kv: kv[1][0]):
        B = args.batch
        pl, pr, pt, pb = (pad,) * 4 if isinstance(pad, int) else pad
        OH, OW = (H + pt + pb - 5) // stride + 1, (W + pl + pr - 5) // stride + 1
        byts = B * C * (H * W + OH * OW) * (4 if dt == torch.float32 else 2) + (B * C * 4 if want_mean else 0)
        n_ring = max(2, -(-args.ring_mib * 2 ** 20 // byts) + 1)
        xs = [torch.randn(B, C, H, W, device='cuda', generator=g).to(dt) for _ in range(n_ring)]
        w = torch.randn(C, 1, 5, 5, device='cuda', generator=g) * 0.2
        b = torch.randn(C, device='cuda', generator=g)
        conv = backbones.DepthwiseConv2d(C, C, 5, stride, pad if isinstance(pad, int) else 0, groups=C, bias=False).cuda().to(dt)
        with torch.no_grad():
            conv.weight.copy_(w)

        def old(x):
            yy = conv(x if isinstance(pad, int) else F.pad(x, (pl, pr, pt, pb)))
            if want_mean:
                return kernels.bias_act_rowmean_(yy, b, act)[0]
            return kernels.bias_act_(yy, b, act)

        def new(x):
            r = kernels.depthwise5x5_bias_act(x, w, b, act, stride, pad, want_mean=want_mean)
            return r[0] if want_mean else r

        def captured(fn):
            """One call of fn per ring buffer as one HIP graph (fn has run eagerly before: lazy set-up is done)."""
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                fn(xs[0])
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    for x in xs:
                        fn(x)
            torch.cuda.current_stream().wait_stream(st)
            torch.cuda.synchronize()
            return graph

        def timed(graph):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            graph.replay()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e3 / n_ring

        med = lambda v: sorted(v)[len(v) // 2]
        with torch.inference_mode():
            a, c = old(xs[0]), new(xs[0])
            torch.cuda.synchronize()
            diff = float((a - c).abs().max().float() / a.abs().max().float().clamp_min(1e-30))
            arm_old, arm_new = captured(old), captured(new)
            for _ in range(2):
                timed(arm_old)
                timed(arm_new)
            t_old, t_new = [], []
            for _ in range(args.rounds):
                t_old.append(timed(arm_old))
                t_new.append(timed(arm_new))
            del arm_old, arm_new
        floor = byts / (HBM_TBS * 1e12) * 1e6
        t, o = med(t_new), med(t_old)
        faster = o - t > max(t_new) - min(t_new)
        row = dict(c=C, hw=f'{H}x{W}', stride=stride, pad=pad, act=act, mean=want_mean, layers=len(names),
                   first=names[0], dtype=args.dtype, batch=B, res=args.res, backbone=args.backbone, ring=n_ring,
                   mbytes=round(byts / 1e6, 1), old_us=round(o, 2), k15_us=round(t, 2), speedup=round(o / t, 3),
                   byte_floor_us=round(floor, 2), k15_share_of_byte_floor=round(floor / t, 3),
                   old_share_of_byte_floor=round(floor / o, 3),
                   k15_us_range=[round(min(t_new), 2), round(max(t_new), 2)],
                   old_us_range=[round(min(t_old), 2), round(max(t_old), 2)], rel_diff=diff,
                   verdict='k15' if faster else 'k15_slower', key=[C, H, W, stride])
        rows.append(row)
        print(json.dumps(row), flush=True)
        del xs
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
