#!/usr/bin/env python
"""Per-shape A/B of the FusedMBConv blocks a 16-bit backbone copy arms with fold_batchnorm(fuse_blocks=True): K16h
(kernels.fused_mbconv16: one launch, the expanded activation kept in LDS) against the chain the default copy runs
for that block today -- the block's own two modules, i.e. K14h or MIOpen + K10 for the 3x3 expand, then K13h or
rocBLAS + K10 for the 1x1 project, as Conv3x3BiasAct.k14h_slower and ConvBiasAct.k13h_slower dispatch them.

    python tools/fused_mbconv_ab.py --out OUT.jsonl      # on the GPU: both networks, both dtypes, one process

The method is tools/conv3x3_ab.py's: the armed blocks and their input shapes are read from a hooked forward; both
arms are the block's forward (FusedMBConv.use_k16h off / on, k16h_slower emptied), each captured as a HIP graph of
--iters calls whose replays are timed with device events, the arms alternated in --rounds rounds; the median per-call
time is reported with the share of the byte floor (one 16-bit read of x, W3 and W1, one write of y, at the measured
6.29 TB/s copy rate of an MI355X).  `slower` is the rule of FusedMBConv.k16h_slower: the fused median loses to the
chain's; a key is listed when that holds in f16 or in bf16 (the last line printed collects them).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_TBS = 6.29
WORKLOADS = [('effnetv2-s', 64, 256), ('effnetv2-l', 32, 384)]


def armed_blocks(net, res):
    """{(Cin, Cmid, Cout, stride, H, W): [module, ...]} of the armed blocks of `net` at `res` px."""
    import torch
    from metrabs_amd import backbones
    out = {}
    hooks = []
    for m in net.modules():
        if isinstance(m, backbones.FusedMBConv) and m.fused_pair:
            def hook(mod, args):
                x = args[0]
                e, p = mod.fused_pair
                key = (e.conv.in_channels, e.conv.out_channels, p.conv.out_channels, e.stride, x.shape[2], x.shape[3])
                out.setdefault(key, []).append(mod)
            hooks.append(m.register_forward_pre_hook(hook))
    backbones.FusedMBConv.use_k16h = False
    try:
        with torch.inference_mode():
            net(torch.rand(1, 3, res, res, device='cuda'))
    finally:
        backbones.FusedMBConv.use_k16h = True
    for h in hooks:
        h.remove()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--dtypes', default='f16,bf16')
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from metrabs_amd import backbones, kernels
    FM = backbones.FusedMBConv
    listed, FM.k16h_slower = FM.k16h_slower, frozenset()   # measure every shape, listed or not
    rows, losers = [], set()

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
    for backbone, B, res in WORKLOADS:
        for dname in args.dtypes.split(','):
            dt = {'f16': torch.float16, 'bf16': torch.bfloat16}[dname]
            net = backbones.fold_batchnorm(backbones.build_backbone(backbone).eval(), fused_epilogue=True, dtype=dt,
                                           fuse_blocks=True).cuda()
            g = torch.Generator(device='cuda').manual_seed(0)
            for key, mods in armed_blocks(net, res).items():
                Cin, Cmid, Cout, stride, H, W = key
                Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
                mod = mods[0]
                e, p = mod.fused_pair
                x = torch.randn(B, Cin, H, W, device='cuda', generator=g).to(dt)
                supported = kernels.fused_mbconv16_supported(x, e.weight_packed, p.conv.weight, stride)

                def arm(on):
                    def fn():
                        FM.use_k16h = on
                        try:
                            return mod(x)
                        finally:
                            FM.use_k16h = True
                    return fn

                chain, fused = arm(False), arm(True)
                with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False,
                                                                        deterministic=False):
                    a = chain()
                    paths = (mod.last_path, e.last_path, p.last_path)
                    assert paths[0] == 'chain'
                    equal = None
                    if supported:
                        c = fused()
                        assert mod.last_path == 'k16h'
                        torch.cuda.synchronize()
                        equal = bool(torch.equal(a, c))
                    for _ in range(3):
                        chain()
                        if supported:
                            fused()
                    arm_old = captured(chain)
                    arm_new = captured(fused) if supported else None
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
                byts = 2 * (B * (H * W * Cin + Ho * Wo * Cout) + 9 * Cmid * Cin + Cout * Cmid)
                mid_mb = 2 * B * Ho * Wo * Cmid / 1e6
                floor = byts / (HBM_TBS * 1e12) * 1e6
                row = dict(backbone=backbone, batch=B, res=res, dtype=dname, cin=Cin, cmid=Cmid, cout=Cout,
                           stride=stride, hw=f'{H}x{W}', skip=mod.residual, layers=len(mods), chain_expand=paths[1],
                           chain_project=paths[2], mbytes=round(byts / 1e6, 1), mid_mbytes=round(mid_mb, 1),
                           chain_us=round(med(t_old), 2), chain_us_range=[round(min(t_old), 2), round(max(t_old), 2)],
                           k16h_us=None, listed=key in listed)
                if supported:
                    t = med(t_new)
                    row.update(k16h_us=round(t, 2), k16h_us_range=[round(min(t_new), 2), round(max(t_new), 2)],
                               speedup=round(med(t_old) / t, 3), byte_floor_us=round(floor, 2),
                               share_of_byte_floor=round(floor / t, 3), equal_bits=equal, slower=t > med(t_old),
                               lds_bytes=int(kernels._lib.load().mtr_fused_mbconv16_lds_bytes(B, Cin, Cmid, Cout, H, W,
                                                                                               stride)))
                    if t > med(t_old):
                        losers.add(key)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del net
            torch.cuda.empty_cache()
    FM.k16h_slower = listed
    print(json.dumps(dict(k16h_slower=sorted(losers))), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')
        f.write(json.dumps(dict(k16h_slower=sorted(losers))) + '\n')


if __name__ == '__main__':
    main()
