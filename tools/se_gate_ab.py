#!/usr/bin/env python
"""Per-shape timing of K12, the squeeze-excite gate (kernels.se_gate, csrc/se.hip): every workgroup split
(config 0 .. 3 and the library's own choice) with the fc2 weight as it is ([C, S]) and transposed ([S, C]).

    python tools/se_gate_ab.py --out OUT.jsonl [--label tree]      # on the GPU

Shapes: the (C, S) of EfficientNetV2-S's squeeze-excite blocks at batch 64 and MobileNetV3-Large's at batch 320
(--shapes C:S:B,... overrides).  Each arm is --iters calls captured in a HIP graph, over --rot rotating sets of
input and output buffers (so no arm re-reads what it has just written), its replays timed with device events, the
arms alternated in --rounds rounds; the median per-call time is reported.  A library that has no
mtr_se_gate_opts (a parent commit) is timed through mtr_se_gate alone: run the tool once in either tree with
--label and set the files side by side.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(256, 16, 64), (512, 32, 64), (768, 32, 64), (960, 40, 64), (1536, 64, 64),
          (72, 18, 320), (120, 30, 320), (480, 120, 320), (672, 168, 320), (960, 240, 320)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--rot', type=int, default=4)
    ap.add_argument('--shapes', default=None)
    ap.add_argument('--label', default='tree')
    ap.add_argument('--out', required=True)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import inspect
    import torch
    from metrabs_amd import kernels
    has_opts = 'config' in inspect.signature(kernels.se_gate).parameters
    shapes = SHAPES if args.shapes is None else [tuple(int(v) for v in s.split(':')) for s in args.shapes.split(',')]
    g = torch.Generator(device='cuda').manual_seed(0)
    rows = []
    for C, S, B in shapes:
        act, gate = ('silu', 'sigmoid') if B == 64 else ('relu', 'hardsigmoid')
        sets = []
        for _ in range(args.rot):
            mean = torch.randn(B, C, device='cuda', generator=g)
            w1 = torch.randn(S, C, device='cuda', generator=g) / C ** 0.5
            b1 = 0.1 * torch.randn(S, device='cuda', generator=g)
            w2 = torch.randn(C, S, device='cuda', generator=g) / S ** 0.5
            b2 = 0.1 * torch.randn(C, device='cuda', generator=g)
            sets.append((mean, w1, b1, w2, b2, w2.t().contiguous(), torch.empty(B, C, device='cuda')))
        arms = {'plain': {}}
        if has_opts:
            arms = {f'{lay}_{cfg}': dict(config=cfg, transposed=lay == 'w2t')
                    for lay in ('w2', 'w2t') for cfg in (-1, 0, 1, 2, 3)}

        def call(i, opt):
            mean, w1, b1, w2, b2, w2t, out = sets[i % args.rot]
            if not has_opts:
                return kernels.se_gate(mean, w1, b1, w2, b2, act, gate, out=out)
            return kernels.se_gate(mean, w1, b1, w2, b2, act, gate, out=out, config=opt['config'],
                                   w2t=w2t if opt['transposed'] else None)

        graphs = {}
        with torch.inference_mode():
            for name, opt in list(arms.items()):
                try:
                    call(0, opt)
                except RuntimeError:   # a split the shape does not fit (LDS, grid)
                    del arms[name]
                    continue
                st = torch.cuda.Stream()
                st.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(st):
                    st.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                        for i in range(args.iters):
                            call(i, opt)
                torch.cuda.current_stream().wait_stream(st)
                torch.cuda.synchronize()
                graphs[name] = graph

            def timed(graph):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                graph.replay()
                ev[1].record()
                torch.cuda.synchronize()
                return ev[0].elapsed_time(ev[1]) * 1e3 / args.iters

            for graph in graphs.values():
                timed(graph), timed(graph)
            times = {name: [] for name in graphs}
            for _ in range(args.rounds):
                for name, graph in graphs.items():
                    times[name].append(timed(graph))
        med = lambda v: sorted(v)[len(v) // 2]
        row = dict(label=args.label, C=C, S=S, B=B, act=act, gate=gate, iters=args.iters, rot=args.rot,
                   us={name: round(med(v), 2) for name, v in times.items()},
                   us_min={name: round(min(v), 2) for name, v in times.items()},
                   us_max={name: round(max(v), 2) for name, v in times.items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
        del graphs
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        for r in rows:
            f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
