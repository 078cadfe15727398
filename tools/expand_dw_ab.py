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

    python tools/expand_dw_ab.py --kernel k26h --out OUT.jsonl

does the same for fold_batchnorm(fuse_expand_depthwise_planes=True), K26h (kernels.expand_depthwise16_planes), on the
384 px planes: EfficientNetV2-L at batch 32 and -S at batch 64.  The chain there is K13h + K11's generic kernel; one
more arm, 'k18', is K13h + K18 (kernels.depthwise3x3_blocks_bias_act, what block_depthwise=True runs for the pair) and
is recorded beside the others.  `slower` and the last line are the rule of DepthwiseBiasAct.k26h_slower, against the
chain; chain_spread is the chain's largest round over its smallest, the noise floor.

    python tools/expand_dw_ab.py --kernel k27h --out OUT.jsonl

is fold_batchnorm(fuse_expand_depthwise_tiles=True), K27h (kernels.expand_depthwise16_tiles), on the three classes of
MobileNetV3 at batch 320 and 256 px it takes: 24 -> 72 on 64x64 at stride 1 (with the 'k18' arm), 16 -> 64 on 128x128 and
40 -> 240 on 32x32 at stride 2.  A key carries the stride as a fifth element, as DepthwiseBiasAct.k27h_slower does; the
byte floor counts x and W1 read once and the (stride-2: four times smaller) y written once.  K27h has one
workgroup-to-image mapping: no 'plain' / 'xcd' arms.

    python tools/expand_dw_ab.py --kernel k28h --out OUT.jsonl

is fold_batchnorm(fuse_expand_depthwise5x5=True), K28h (kernels.expand_depthwise16_k5), on the 5x5 pairs of MobileNetV3
at batch 320 and 256 px: the chain is K13h + K15 with the squeeze-excite mean.  The key carries the stride, as
DepthwiseBiasAct.k28h_slower does; the 24 -> 72 pair on 64x64 at stride 2 is outside K28h's LDS rule and is recorded with
the chain's time alone.  The 'plain' / 'xcd' arms pass the stride and the mean.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_TBS = 6.29
# per kernel, beside what backbones.EXPAND_DW_KERNELS says of it (option, field, switch, slower, takes, fn, strided): the
# LDS query and the (backbone, batch, px) measured
KERNELS = {
    'k25h': dict(lds='mtr_expand_dw16_lds_bytes', workloads=[('effnetv2-s', 64, 256), ('mobilenetv3', 320, 256)]),
    'k26h': dict(lds='mtr_expand_dw16_planes_lds_bytes', workloads=[('effnetv2-l', 32, 384), ('effnetv2-s', 64, 384)]),
    'k27h': dict(lds='mtr_expand_dw16_tiles_lds_bytes', workloads=[('mobilenetv3', 320, 256)]),
    'k28h': dict(lds='mtr_expand_dw16_k5_lds_bytes', workloads=[('mobilenetv3', 320, 256)]),
}


def armed_pairs(net, res, cfg):
    """{(Cin, Cmid, H, W): [(expand, depthwise), ...]} of the armed pairs of `net` at `res` px (cfg['strided']: the
    depthwise layer's stride as a fifth element of the key)."""
    import torch
    from metrabs_amd import backbones
    out = {}
    hooks = []
    for m in net.modules():
        if isinstance(m, backbones.ConvBiasAct) and getattr(m, cfg['field']):
            def hook(mod, args):
                x = args[0]
                dw = getattr(mod, cfg['field'])[0]
                key = (mod.conv.in_channels, mod.conv.out_channels, x.shape[2], x.shape[3])
                out.setdefault(key + ((dw.stride,) if cfg['strided'] else ()), []).append((mod, dw))
            hooks.append(m.register_forward_pre_hook(hook))
    setattr(backbones.DepthwiseBiasAct, cfg['switch'], False)
    try:
        with torch.inference_mode():
            net(torch.rand(1, 3, res, res, device='cuda'))
    finally:
        setattr(backbones.DepthwiseBiasAct, cfg['switch'], True)
    for h in hooks:
        h.remove()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--dtypes', default='f16,bf16')
    ap.add_argument('--kernel', choices=sorted(KERNELS), default='k25h')
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    kn = args.kernel
    sys.path.insert(0, ROOT)
    import torch
    from metrabs_amd import backbones, kernels
    cfg = dict(backbones.EXPAND_DW_KERNELS[kn], **KERNELS[kn])
    DW = backbones.DepthwiseBiasAct
    listed = getattr(DW, cfg['slower'])
    setattr(DW, cfg['slower'], frozenset())   # measure every shape, listed or not
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
    for backbone, B, res in cfg['workloads']:
        for dname in args.dtypes.split(','):
            dt = {'f16': torch.float16, 'bf16': torch.bfloat16}[dname]
            net = backbones.fold_batchnorm(backbones.build_backbone(backbone).eval(), fused_epilogue=True, dtype=dt,
                                           **{cfg['option']: True}).cuda()
            g = torch.Generator(device='cuda').manual_seed(0)
            for key, pairs in armed_pairs(net, res, cfg).items():
                Cin, Cmid, H, W = key[:4]
                e, d = pairs[0]
                stride = d.stride
                if kn == 'k27h' and (stride == 1 and kernels.k11_takes_block_kernel(H, W) or d.emit_mean):
                    continue   # (the 16x16 pairs: not K27h's planes)
                x = torch.randn(B, Cin, H, W, device='cuda', generator=g).to(dt)

                def chain():
                    return d(e.forward_here(x))

                def fused():
                    return d(e(x))

                def mapped(mapping):
                    extra = dict(stride=stride) if cfg['strided'] else {}
                    return lambda: getattr(kernels, cfg['fn'])(x, e.conv.weight, e.bias, e.act_name, d.weight, d.bias,
                                                               d.act_name, want_mean=d.emit_mean, mapping=mapping,
                                                               **extra)

                def k18():
                    return kernels.depthwise3x3_blocks_bias_act(e.forward_here(x), d.weight, d.bias, d.act_name,
                                                                want_mean=d.emit_mean)

                with torch.inference_mode():
                    a = chain()
                    chain_paths = (e.last_path, d.last_path)
                    supported = getattr(d, cfg['takes'])(x, e)
                    arms = {'chain': chain}
                    equal = None
                    if kn == 'k26h' or (kn == 'k27h' and stride == 1):
                        arms['k18'] = k18
                    if supported:
                        c = fused()
                        assert (e.last_path, d.last_path) == (kn, kn)
                        torch.cuda.synchronize()
                        equal = bool(torch.equal(a, c))
                        arms[kn] = fused
                        if kn != 'k27h':
                            arms.update(plain=mapped('plain'), xcd=mapped('xcd'))
                    for _ in range(3):
                        for fn in arms.values():
                            fn()
                    graphs = {n: captured(fn) for n, fn in arms.items()}
                    for _ in range(2):
                        for gr in graphs.values():
                            timed(gr)
                    t = {n: [] for n in graphs}
                    for _ in range(args.rounds):   # alternated: chain, (k18,) the kernel, plain, xcd, chain, ...
                        for n, gr in graphs.items():
                            t[n].append(timed(gr))
                    del graphs
                byts = 2 * (B * H * W * Cin + B * (-(-H // stride)) * (-(-W // stride)) * Cmid + Cmid * Cin)
                mid_mb = 2 * B * H * W * Cmid / 1e6
                floor = byts / (HBM_TBS * 1e12) * 1e6
                row = dict(backbone=backbone, batch=B, res=res, dtype=dname, cin=Cin, cmid=Cmid, hw=f'{H}x{W}',
                           act=e.act_name, stride=stride, mean=d.emit_mean, layers=len(pairs), chain_expand=chain_paths[0],
                           chain_depthwise=chain_paths[1], mbytes=round(byts / 1e6, 1), mid_mbytes=round(mid_mb, 1),
                           chain_us=round(med(t['chain']), 2), chain_us_rounds=[round(v, 2) for v in t['chain']],
                           listed=key in listed, **{kn + '_us': None})
                if 'k18' in t:
                    row.update(chain_spread=round(max(t['chain']) / min(t['chain']), 4),
                               k18_us=round(med(t['k18']), 2), k18_us_rounds=[round(v, 2) for v in t['k18']])
                if supported:
                    tk = med(t[kn])
                    ahead_every_round = all(n < o for n, o in zip(t[kn], t['chain']))
                    row.update({kn + '_us': round(tk, 2), kn + '_us_rounds': [round(v, 2) for v in t[kn]]})
                    if 'plain' in t:
                        row.update(plain_us_rounds=[round(v, 2) for v in t['plain']],
                                   xcd_us_rounds=[round(v, 2) for v in t['xcd']])
                    row.update(
                               speedup=round(med(t['chain']) / tk, 3), byte_floor_us=round(floor, 2),
                               share_of_byte_floor=round(floor / tk, 3), equal_bits=equal,
                               slower=not ahead_every_round,
                               lds_bytes=int(getattr(kernels._lib.load(), cfg['lds'])(
                                   B, Cin, Cmid, H, W, *((stride,) if cfg['strided'] else ()))))
                    if not ahead_every_round:
                        losers.add(key)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del net
            torch.cuda.empty_cache()
    setattr(DW, cfg['slower'], listed)
    print(json.dumps({cfg['slower']: sorted(losers)}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')
        f.write(json.dumps({cfg['slower']: sorted(losers)}) + '\n')


if __name__ == '__main__':
    main()
