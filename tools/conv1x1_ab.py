#!/usr/bin/env python
"""Per-shape A/B of the 1x1 convolutions of EfficientNetV2-S at the bench shape (batch 64, 256 px, f32):
K13 (kernels.conv1x1_bias_act: one launch) against the path it replaces (x * gate where a squeeze-excite
block hands one over, the library convolution under the deterministic pin bench.py uses, K10).
--dtype f16 / bf16 times K13h (kernels.conv1x1_bias_act16) against rocBLAS f16 / bf16 + K10 (+ x * gate) on
16-bit tensors instead; --backbone / --batch / --res pick the network and shape (effnetv2-l, 32, 384: configs[4]).

    python tools/conv1x1_ab.py --out OUT.jsonl      # on the GPU

Shapes are read from a hooked forward of the folded network; each class (Cin, Cout, H, W, act, skip,
gate) is timed with device events over --iters calls per arm, the two arms alternated in rounds, and
reported as the median per-call time with its share of the MFMA peak (155 TF f32, 2.5 PF f16 / bf16) and of
the HBM floor (one read of x, w and the skip, one write of y, at HBM_TBS: the measured copy bandwidth of an
MI355X, 6.29 TB/s; the spec is 8.0).
--config lists the configurations to time (f32: kernels.CONV1X1_CONFIGS, 16 bits: kernels.CONV1X1_16_CONFIGS); --deep
keeps the deep project classes only (no activation, Cin >= 768, Cout > 160: what fold_batchnorm(deep_projects=True)
arms), e.g. --dtype f16 --deep --config deepk,auto: the library chain, K13h 'deepk' and K13h's own choice.
--timing graph (the 16-bit default) captures --iters calls of each arm in a HIP graph and times its replays:
GPU time without the host's launch cost, as the estimator runs its graphed batches.  --timing eager (the f32
default) times the calls as they are issued.  The library arm of a 16-bit run is unpinned (cudnn deterministic
off), as the 16-bit copy runs by default; the f32 arm keeps the deterministic pin the f32 model runs under.
The projects of the FusedMBConv blocks an f32 copy arms (FusedMBConv.pre_pair: the dense 3x3 in front leaves its K10
pass to them) are timed as that hand-over: old = K10 in place on the expanded activation, then K13; new = K13 with
the input prologue (in_bias, in_act), one launch and one read and one write of the activation less.  --only-pre
times these classes alone.
--ab k20 (f32 only) times K13 ('auto', with the prologue where the class has one) against K20
(kernels.conv1x1_bias_act_split: the same call on the bf16 matrix cores from split operands) per class: HIP graphs of
--iters calls (default 20 in this mode), --rounds alternated rounds, medians, every round kept, with K20's share of the
byte floor and of the six-product matrix ceiling (2.5 PF / 6), and the error of both against fp64.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_TF, PEAK16_TF, HBM_TBS = 155.0, 2500.0, 6.29


def shape_classes(batch, res, backbone='effnetv2-s'):
    import torch
    from metrabs_amd import backbones
    net = backbones.fold_batchnorm(backbones.build_backbone(backbone).eval(), fused_epilogue=True).cuda()
    out = {}
    pre_of = {m.pre_pair[1]: m.pre_pair[0] for m in net.modules()
              if isinstance(m, backbones.FusedMBConv) and m.pre_pair}
    for name, m in net.named_modules():
        if isinstance(m, backbones.ConvBiasAct) and m.conv.kernel_size == (1, 1) and m.conv.stride == (1, 1):
            def hook(mod, args, kwargs, name=name):
                x = args[0]
                gated = any(mod in se.gate_to for se in net.modules() if isinstance(se, backbones.SqueezeExcite))
                key = (x.shape[1], mod.conv.out_channels, x.shape[2], x.shape[3], mod.act_name,
                       kwargs.get('residual') is not None, gated, pre_of[mod].act_name if mod in pre_of else False)
                out.setdefault(key, []).append(name)
            m.register_forward_pre_hook(hook, with_kwargs=True)
    backbones.ConvBiasAct.use_k13 = False
    with torch.inference_mode():
        net(torch.rand(1, 3, res, res, device='cuda'))
    backbones.ConvBiasAct.use_k13 = True
    return out


def k20_ab(args, classes):
    """The --ab k20 arm: K13 'auto' against K20 per class, both as HIP graph replays."""
    import torch
    from metrabs_amd import kernels
    g = torch.Generator(device='cuda').manual_seed(0)
    B, rows = args.batch, []
    med = lambda v: sorted(v)[len(v) // 2]
    for (K, M, H, W, act, res, gated, pre_act), names in sorted(classes.items(), key=lambda kv: kv[1][0]):
        if args.max_hw is not None and H * W > args.max_hw:
            continue
        pre = pre_act is not False
        x = torch.randn(B, K, H, W, device='cuda', generator=g)
        w = torch.randn(M, K, 1, 1, device='cuda', generator=g) / K ** 0.5
        b = torch.randn(M, device='cuda', generator=g)
        gate = torch.rand(B, K, device='cuda', generator=g) if gated else None
        r = torch.randn(B, M, H, W, device='cuda', generator=g) if res else None
        b_in = torch.randn(K, device='cuda', generator=g) if pre else None
        ws = kernels.pack_conv1x1_split_weight(w)
        if not (kernels.conv1x1_supported(x, w) and kernels.conv1x1_split_supported(x, ws)):
            continue
        y13, y20 = (torch.empty(B, M, H, W, device='cuda') for _ in range(2))
        kw = dict(gate=gate, residual=r, in_bias=b_in, in_act=pre_act if pre else None)
        k13 = lambda: kernels.conv1x1_bias_act(x, w, b, act, out=y13, **kw)
        k20 = lambda: kernels.conv1x1_bias_act_split(x, ws, b, act, out=y20, **kw)

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

        with torch.inference_mode():
            k13(), k20()
            # the error of both against fp64, on the GEMM alone (the first image: enough elements, a small reference)
            xg = kernels.bias_act_(x[:1].clone(), b_in, pre_act) if pre else x[:1]
            xg = xg if gate is None else xg * gate[:1, :, None, None]
            ref = torch.einsum('mk,bkhw->bmhw', w.double().flatten(1), xg.double())
            zero = torch.zeros_like(b)
            rms = lambda t: float(((t.double() - ref) ** 2).mean().sqrt() / (ref ** 2).mean().sqrt())
            e13 = rms(kernels.conv1x1_bias_act(xg, w, zero, None))
            e20 = rms(kernels.conv1x1_bias_act_split(xg, ws, zero, None))
            g13, g20 = captured(k13), captured(k20)
            for _ in range(2):
                timed(g13), timed(g20)
            t13, t20 = [], []
            for _ in range(args.rounds):
                t13.append(timed(g13))
                t20.append(timed(g20))
            del g13, g20
        flop = 2.0 * B * H * W * K * M
        byts = 4 * (B * H * W * (K + M * (2 if res else 1))) + 6 * M * K
        byte_floor = byts / (HBM_TBS * 1e12) * 1e6
        mfma_floor = flop / (PEAK16_TF / 6 * 1e12) * 1e6
        row = dict(ab='k20', cin=K, cout=M, hw=f'{H}x{W}', act=act, skip=res, gate=gated, pre_act=pre_act,
                   layers=len(names), first=names[0], batch=B, res=args.res, backbone=args.backbone, iters=args.iters,
                   k13_plan=list(kernels.conv1x1_plan(M, K, H * W, B)), k13_us=round(med(t13), 2),
                   k20_us=round(med(t20), 2), k13_rounds=[round(v, 2) for v in t13],
                   k20_rounds=[round(v, 2) for v in t20], k20_ahead_every_round=all(n < o for n, o in zip(t20, t13)),
                   speedup=round(med(t13) / med(t20), 3), byte_floor_us=round(byte_floor, 2),
                   k20_share_of_byte_floor=round(byte_floor / med(t20), 3), mfma6_floor_us=round(mfma_floor, 2),
                   k20_share_of_mfma6=round(mfma_floor / med(t20), 3), hbm_tbs=HBM_TBS,
                   k13_rel_rms=e13, k20_rel_rms=e20)
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
    ap.add_argument('--iters', type=int, default=None, help='calls per timed arm (default 50; 20 with --ab k20)')
    ap.add_argument('--ab', choices=['k20'], default=None,
                    help='k20 (f32): K13 as it dispatches against K20, the split-operand kernel, per class')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--dtype', choices=['f32', 'f16', 'bf16'], default='f32')
    ap.add_argument('--backbone', default='effnetv2-s')
    ap.add_argument('--timing', choices=['graph', 'eager'], default=None,
                    help='default: graph for f16 / bf16, eager for f32')
    ap.add_argument('--config', default='auto', help='K13 / K13h configurations to time, comma-separated; the first is the "new" arm, each further one is '
                         'timed beside it and compared with it round by round (--config tall,stream: the streaming '
                         'configuration against the tall tiles)')
    ap.add_argument('--max-hw', type=int, default=None)
    ap.add_argument('--only-pre', action='store_true', help='the FusedMBConv projects that take the prologue only')
    ap.add_argument('--deep', action='store_true', help='the deep project classes only (no activation, Cin >= 768, Cout > 160)')
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    from metrabs_amd import kernels
    args.iters = args.iters or (20 if args.ab else 50)
    classes = shape_classes(args.batch, args.res, args.backbone)
    if args.ab == 'k20':
        if args.dtype != 'f32':
            ap.error('--ab k20 needs --dtype f32')
        return k20_ab(args, classes)
    dt = {'f32': torch.float32, 'f16': torch.float16, 'bf16': torch.bfloat16}[args.dtype]
    k = 'k13' if dt == torch.float32 else 'k13h'
    peak = PEAK_TF if dt == torch.float32 else PEAK16_TF
    timing = args.timing or ('eager' if dt == torch.float32 else 'graph')
    pinned = dt == torch.float32
    rows = []
    configs = args.config.split(',')
    g = torch.Generator(device='cuda').manual_seed(0)
    for (K, M, H, W, act, res, gated, pre_act), names in sorted(classes.items(), key=lambda kv: kv[1][0]):
        if args.max_hw is not None and H * W > args.max_hw:
            continue
        pre = pre_act is not False and dt == torch.float32
        if args.only_pre and not pre:
            continue
        if args.deep and not (act is None and K >= 768 and M > 160):
            continue
        B = args.batch
        x = torch.randn(B, K, H, W, device='cuda', generator=g).to(dt)
        w = (torch.randn(M, K, 1, 1, device='cuda', generator=g) / K ** 0.5).to(dt)
        b = torch.randn(M, device='cuda', generator=g)
        gate = torch.rand(B, K, device='cuda', generator=g) if gated else None
        r = torch.randn(B, M, H, W, device='cuda', generator=g).to(dt) if res else None
        y = torch.empty(B, M, H, W, device='cuda', dtype=dt)
        b_in = torch.randn(K, device='cuda', generator=g) if pre else None

        def old():
            if pre:   # (K10 works in place: the values of x change from call to call, the time does not)
                kernels.bias_act_(x, b_in, pre_act)
                return kernels.conv1x1_bias_act(x, w, b, act, gate=gate, residual=r, out=y)
            xi = x if gate is None else x * gate.to(dt).view(B, K, 1, 1)
            yy = F.conv2d(xi, w)
            kernels.bias_act_(yy, b, act, r)
            return yy

        def new(config=configs[0]):
            if dt != torch.float32:
                return kernels.conv1x1_bias_act16(x, w, b, act, gate=gate, residual=r, out=y, config=config)
            return kernels.conv1x1_bias_act(x, w, b, act, gate=gate, residual=r, out=y, config=config, in_bias=b_in,
                                            in_act=pre_act if pre else None)

        extra = {c: (lambda c=c: new(c)) for c in configs[1:]}

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

        def timed(fn):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            if timing == 'graph':
                fn.replay()
            else:
                for _ in range(args.iters):
                    fn()
            ev[1].record()
            torch.cuda.synchronize()
            return ev[0].elapsed_time(ev[1]) * 1e3 / args.iters

        with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=pinned):
            if pre:
                x0 = x.clone()
                c = new().clone()
                a = old().clone()
                assert torch.equal(a, c)   # the prologue has K10's bits
                x.copy_(x0)
            else:
                a, c = old(), new()
            torch.cuda.synchronize()
            diff = float((a - c).abs().max().float() / a.abs().max().float().clamp_min(1e-30))
            for fn in extra.values():
                assert torch.equal(fn().clone(), c)   # every configuration returns the same bits
            for _ in range(3):
                old(), new()
            arm_old, arm_new = (captured(old), captured(new)) if timing == 'graph' else (old, new)
            arm_extra = {c: captured(fn) if timing == 'graph' else fn for c, fn in extra.items()}
            for _ in range(2):
                timed(arm_old), timed(arm_new)
                for fn in arm_extra.values():
                    timed(fn)
            t_old, t_new, t_extra = [], [], {c: [] for c in extra}
            for _ in range(args.rounds):
                t_old.append(timed(arm_old))
                t_new.append(timed(arm_new))
                for c, fn in arm_extra.items():
                    t_extra[c].append(timed(fn))
            del arm_old, arm_new, arm_extra
        med = lambda v: sorted(v)[len(v) // 2]
        flop = 2.0 * B * H * W * K * M
        byts = x.element_size() * (B * H * W * (K + M * (2 if res else 1)) + M * K)
        byte_floor = byts / (HBM_TBS * 1e12) * 1e6
        floor = max(flop / (peak * 1e12) * 1e6, byte_floor)
        # (the old arm of a prologue class reads and writes x once more)
        byts_old = byts + (x.element_size() * 2 * B * K * H * W if pre else 0)
        row = dict(cin=K, cout=M, hw=f'{H}x{W}', act=act, skip=res, gate=gated, layers=len(names), first=names[0],
                   **(dict(pre_act=pre_act, old='k10+k13', old_floor_us=round(byts_old / (HBM_TBS * 1e12) * 1e6, 2),
                           old_rounds=[round(v, 2) for v in t_old], new_rounds=[round(v, 2) for v in t_new])
                      if pre else {}),
                   old_us=round(med(t_old), 2), **{f'{k}_us': round(med(t_new), 2),
                                                   f'{k}_tflops': round(flop / med(t_new) / 1e6, 1),
                                                   f'{k}_share_of_peak': round(flop / med(t_new) / 1e6 / peak, 3)},
                   floor_us=round(floor, 2), speedup=round(med(t_old) / med(t_new), 3), rel_diff=diff)
        plan = kernels.conv1x1_plan if dt == torch.float32 else kernels.conv1x1_16_plan
        if dt == torch.float32 or args.config != 'auto':
            row.update(config=configs[0], plan=list(plan(M, K, H * W, B, configs[0])), timing=timing,
                       wins_every_round=all(n < o for n, o in zip(t_new, t_old)))
            if dt != torch.float32:
                row.update(old_rounds=[round(v, 2) for v in t_old], new_rounds=[round(v, 2) for v in t_new])
            for c, v in t_extra.items():
                row[f'{k}_{c}_us'] = round(med(v), 2)
                row[f'{k}_{c}_plan'] = list(plan(M, K, H * W, B, c))
                row[f'{k}_{c}_wins_every_round'] = all(n < o for n, o in zip(v, t_old))
                row[f'{k}_{c}_rounds'] = [round(t, 2) for t in v]
                row[f'{c}_beats_{configs[0]}_every_round'] = all(n < o for n, o in zip(v, t_new))
        if dt != torch.float32:
            row.update(dtype=args.dtype, batch=B, res=args.res, timing=timing, library_pinned=pinned, hbm_tbs=HBM_TBS,
                       byte_floor_us=round(byte_floor, 2), share_of_byte_floor=round(byte_floor / med(t_new), 3))
        rows.append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
