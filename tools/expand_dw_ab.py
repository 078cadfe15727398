#!/usr/bin/env python
"""Per-shape A/B of the (1x1 expand, depthwise 3x3) pairs a 16-bit backbone copy arms with
fold_batchnorm(fuse_expand_depthwise=True): K25h (kernels.expand_depthwise16: one launch, the expanded activation kept
in LDS) against the chain the default copy runs for the pair today -- the pair's own two modules, i.e. K13h (or
rocBLAS + K10 for the shapes of ConvBiasAct.k13h_slower) and then K11 with the squeeze-excite mean.

    python tools/expand_dw_ab.py --out OUT.jsonl      # on the GPU: both networks, both dtypes, one process

The method is tools/fused_mbconv_ab.py's: the armed pairs and their input shapes are read from a hooked forward; both
arms are the two modules' forwards (DepthwiseBiasAct.use_k25h off / on, k25h_slower emptied), each captured as a HIP
graph of --iters calls whose replays are timed with device events, the arms alternated in --rounds rounds.  EVERY round
is written out, with the median and the share of the byte floor (one 16-bit read of x and W1, one write of y, at the
measured 6.29 TB/s copy rate of an MI355X).  `slower` is the rule of DepthwiseBiasAct.k25h_slower: K25h is NOT ahead of
the chain in every round; a key is listed when that holds in f16 or in bf16 (the last line printed collects them).
K25h's two workgroup-to-image mappings ('plain', 'xcd') are timed the same way as a third and fourth arm
(kernels.expand_depthwise16(mapping=)); the library's own choice is whichever the entry resolves -1 to.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_TBS = 6.29
WORKLOADS = [('effnetv2-s', 64, 256), ('mobilenetv3', 320, 256)]


def armed_pairs(net, res):
    """{(Cin, Cmid, H, W): [(expand, depthwise), ...]} of the armed pairs of `net` at `res` px."""
    import torch
    from metrabs_amd import backbones
    out = {}
    hooks = []
    for m in net.modules():
        if isinstance(m, backbones.ConvBiasAct) and m.hand_to:
            def hook(mod, args):
                x = args[0]
                key = (mod.conv.in_channels, mod.conv.out_channels, x.shape[2], x.shape[3])
                out.setdefault(key, []).append((mod, mod.hand_to[0]))
            hooks.append(m.register_forward_pre_hook(hook))
    backbones.DepthwiseBiasAct.use_k25h = False
    try:
        with torch.inference_mode():
            net(torch.rand(1, 3, res, res, device='cuda'))
    finally:
        backbones.DepthwiseBiasAct.use_k25h = True
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
    DW = backbones.DepthwiseBiasAct
    listed, DW.k25h_slower = DW.k25h_slower, frozenset()   # measure every shape, listed or not
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
                                           fuse_expand_depthwise=True).cuda()
            g = torch.Generator(device='cuda').manual_seed(0)
            for key, pairs in armed_pairs(net, res).items():
                Cin, Cmid, H, W = key
                e, d = pairs[0]
                x = torch.randn(B, Cin, H, W, device='cuda', generator=g).to(dt)

                def chain():
                    return d(e.forward_here(x))

                def fused():
                    return d(e(x))

                def mapped(mapping):
                    return lambda: kernels.expand_depthwise16(x, e.conv.weight, e.bias, e.act_name, d.weight, d.bias,
                                                              d.act_name, want_mean=d.emit_mean, mapping=mapping)

                with torch.inference_mode():
                    a = chain()
                    chain_paths = (e.last_path, d.last_path)
                    supported = d.k25h_takes(x, e)
                    arms = {'chain': chain}
                    equal = None
                    if supported:
                        c = fused()
                        assert (e.last_path, d.last_path) == ('k25h', 'k25h')
                        torch.cuda.synchronize()
                        equal = bool(torch.equal(a, c))
                        arms.update(k25h=fused, plain=mapped('plain'), xcd=mapped('xcd'))
                    for _ in range(3):
                        for fn in arms.values():
                            fn()
                    graphs = {n: captured(fn) for n, fn in arms.items()}
                    for _ in range(2):
                        for gr in graphs.values():
                            timed(gr)
                    t = {n: [] for n in graphs}
                    for _ in range(args.rounds):   # alternated: chain, k25h, plain, xcd, chain, ...
                        for n, gr in graphs.items():
                            t[n].append(timed(gr))
                    del graphs
                byts = 2 * (B * H * W * (Cin + Cmid) + Cmid * Cin)
                mid_mb = 2 * B * H * W * Cmid / 1e6
                floor = byts / (HBM_TBS * 1e12) * 1e6
                row = dict(backbone=backbone, batch=B, res=res, dtype=dname, cin=Cin, cmid=Cmid, hw=f'{H}x{W}',
                           act=e.act_name, mean=d.emit_mean, layers=len(pairs), chain_expand=chain_paths[0],
                           chain_depthwise=chain_paths[1], mbytes=round(byts / 1e6, 1), mid_mbytes=round(mid_mb, 1),
                           chain_us=round(med(t['chain']), 2), chain_us_rounds=[round(v, 2) for v in t['chain']],
                           k25h_us=None, listed=key in listed)
                if supported:
                    tk = med(t['k25h'])
                    ahead_every_round = all(n < o for n, o in zip(t['k25h'], t['chain']))
                    row.update(k25h_us=round(tk, 2), k25h_us_rounds=[round(v, 2) for v in t['k25h']],
                               plain_us_rounds=[round(v, 2) for v in t['plain']],
                               xcd_us_rounds=[round(v, 2) for v in t['xcd']],
                               speedup=round(med(t['chain']) / tk, 3), byte_floor_us=round(floor, 2),
                               share_of_byte_floor=round(floor / tk, 3), equal_bits=equal,
                               slower=not ahead_every_round,
                               lds_bytes=int(kernels._lib.load().mtr_expand_dw16_lds_bytes(B, Cin, Cmid, H, W)))
                    if not ahead_every_round:
                        losers.add(key)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del net
            torch.cuda.empty_cache()
    DW.k25h_slower = listed
    print(json.dumps(dict(k25h_slower=sorted(losers))), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')
        f.write(json.dumps(dict(k25h_slower=sorted(losers))) + '\n')


if __name__ == '__main__':
    main()
