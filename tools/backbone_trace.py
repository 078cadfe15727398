#!/usr/bin/env python
"""Per-layer kernel times of ONE backbone forward at the bench shape, attributed to blocks and roles.

    # on the GPU: record a marked forward under the kernel tracer
    rocprofv3 --kernel-trace --output-format csv -d OUT/trace -o bb -- \\
        python tools/backbone_trace.py record --markers OUT/markers.json
    # anywhere: the table
    python tools/backbone_trace.py report --trace OUT/trace --markers OUT/markers.json --out TABLE.md

`record` builds the backbone of bench.py's configs[1] the way bench.py:build_model does (EfficientNetV2-S,
batch norm calibrated on the sampler's crops, fold_batchnorm(fused_epilogue=True), f32, the deterministic
convolution pin of Metrabs.deterministic_backbone), runs a few unmarked forwards at batch 64 / 256 px and
then one forward in which a forward pre-hook on every module first launches a marker kernel
(torch.cuda._sleep(0), `spin_kernel`).  The kernels between two markers belong to the module entered
last; `report` names each kernel's role in its block (SE fc1 / bias / act, fc2, gate, mul, project,
K10, K11, se_gate, ...) from that module and the kernel's name and writes a markdown table: per MBConv
block the time of every role, the sum of the squeeze-excite tail, per project shape the GEMM time, and per
depthwise layer (k, C, map, stride) its convolution kernel + K10, or K11 / K15 (`record --no-k15`: the 5x5
layers folded as before K15; `record --no-k13-pre`: the K10 pass behind the dense 3x3 layers of stages 2 - 3, which
the f32 copy otherwise leaves to the project's K13 launch, so that the K10 column of those blocks is empty).  The
block tables are EfficientNetV2's; other backbones (`--backbone mobilenetv3
--batch 320`: configs[3]) get the depthwise table and the split by kernel kind.
Marker kernels and the gaps they open are not counted; kernel durations are the tracer's.
`record --precision` picks the arithmetic: f32 (the default, as above), f16-autocast / bf16-autocast (the f32
copy under torch.autocast, 16-bit crops: bench.py's --precision f16 / bf16), f16-copy / bf16-copy (the 16-bit
copy, fold_batchnorm(dtype=), 16-bit crops; unpinned like 16-bit autocast); `--backbone` / `--batch` / `--res`
the network and shape (effnetv2-l, 32, 384: configs[4]); `record --deep-projects` folds a -copy precision with
deep_projects=True (the deep project convolutions on K13h's deep-K configuration: their x * gate, gemm, K10 and cast
columns are empty).
"""
import argparse
import contextlib
import csv
import glob
import json
import os
import re
import sys
from collections import OrderedDict, defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = 'spin_kernel'


def record(args):
    import types
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from metrabs_amd.backbones import (ConvBiasAct, DepthwiseBiasAct, DepthwiseConv2d, build_backbone,
                                       calibrate_batchnorm, fold_batchnorm)
    if args.no_k13_pre:   # the armed FusedMBConv blocks of the f32 copy on the chain: K10 behind every dense 3x3
        from metrabs_amd.backbones import FusedMBConv
        FusedMBConv.use_k13_pre = False
    if args.no_k15:   # the module tree from before K15: 5x5 depthwise layers as DepthwiseConv2d + K10
        DepthwiseBiasAct.kernel_sizes = (3,)
    dev = torch.device('cuda')
    torch.manual_seed(1234)
    dt = {'f32': None, 'f16': torch.float16, 'bf16': torch.bfloat16}[args.precision.split('-')[0]]
    # Metrabs.deterministic_backbone: pinned for f32 only
    torch.backends.cudnn.deterministic = dt is None
    net = build_backbone(args.backbone).to(dev)
    calibrate_batchnorm(net, args.res, dev,
                        samples=bench.synthetic_crops(types.SimpleNamespace(res=args.res, num_aug=1), dev))
    net = fold_batchnorm(net.eval(), fused_epilogue=True,
                         dtype=dt if args.precision.endswith('-copy') else None, fuse_blocks=args.fuse_blocks,
                         fuse_stem=args.fuse_stem, block_depthwise=args.block_depthwise,
                         winograd3x3=args.winograd3x3, split_gemm=args.split_gemm, strided3x3=args.strided3x3,
                         deep_projects=args.deep_projects, split3x3=args.split3x3)
    x = torch.rand(args.batch, 3, args.res, args.res, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    if dt is not None:
        x = x.to(dt)   # the sampler writes 16-bit crops in both 16-bit modes
    # a fresh autocast region per forward, as Metrabs.forward enters one per call: autocast caches the weight
    # casts of a region, so a region around several forwards would hide them from all but the first
    mode = ((lambda: torch.autocast('cuda', dtype=dt)) if args.precision.endswith('-autocast')
            else contextlib.nullcontext)
    order = []

    depthwise, dw_maps = {}, {}

    def hook(name):
        def pre(mod, inp):
            torch.cuda._sleep(0)
            order.append(name)
            if inp and hasattr(inp[0], 'shape') and inp[0].dim() == 4:
                dw_maps[name] = f'{inp[0].shape[2]}x{inp[0].shape[3]}'
        return pre

    with torch.inference_mode():
        for _ in range(args.warmup):
            with mode():
                net(x)
        torch.cuda.synchronize()
        handles = [m.register_forward_pre_hook(hook(n or '<root>')) for n, m in net.named_modules()]
        with mode():
            feat = net(x)
        torch.cuda.synchronize()
        for h in handles:
            h.remove()
    shapes = {}
    for n, m in net.named_modules():  # depthwise layers for the report: kernel size, channels, input map, stride
        if isinstance(m, DepthwiseBiasAct):
            depthwise[n] = [m.k, m.weight.shape[0], dw_maps.get(n), m.stride]
        elif isinstance(m, ConvBiasAct) and isinstance(m.conv, DepthwiseConv2d):
            depthwise[n] = [m.conv.kernel_size[0], m.conv.in_channels, dw_maps.get(n), m.conv.stride[0]]
    for n, m in net.named_modules():  # 1x1 conv shapes for the report
        if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (1, 1) and m.groups == 1:
            shapes[n] = [m.in_channels, m.out_channels]
    os.makedirs(os.path.dirname(os.path.abspath(args.markers)), exist_ok=True)
    with open(args.markers, 'w') as f:
        json.dump(dict(order=order, conv1x1=shapes, depthwise=depthwise, batch=args.batch, res=args.res,
                       feature_shape=list(feat.shape), precision=args.precision, backbone=args.backbone), f)
    print(f'recorded {len(order)} markers')


def _kernels(trace_dir):
    paths = glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True)
    if not paths:
        raise SystemExit(f'no *kernel_trace.csv under {trace_dir}')
    rows = []
    for p in paths:
        with open(p) as f:
            for r in csv.DictReader(f):
                rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']))
    rows.sort()
    return rows


def _kind(kname):
    k = kname.lower()
    if MARK in k:
        return 'marker'
    if 'se_gate' in k:
        return 'se_gate'
    if 'stem_conv_kernel' in k:  # K17 (before the generic 'conv' match): Preproc + the stem 3x3 stride-2 conv + epilogue
        return 'K17'
    if 'fused_mbconv16_kernel' in k:  # K16h: a whole FusedMBConv block (3x3 expand + 1x1 project) of the 16-bit copy
        return 'K16h'
    if 'conv3x3s2_kernel' in k:  # K22 (before the generic 'conv' match): the f32 dense 3x3 stride-2 conv + epilogue
        return 'K22'
    if 'conv3x3_split_kernel' in k:  # K21 (before the generic 'conv' match): the f32 dense 3x3 conv on the bf16 matrix cores
        return 'K21'
    if 'conv3x3_winograd_kernel' in k:  # K19 (before the generic 'conv' match): the f32 dense 3x3 Winograd conv + epilogue
        return 'K19'
    if 'conv3x3_16_kernel' in k:  # K14h (before the generic 'conv' match): the 16-bit dense 3x3 conv + epilogue
        return 'K14h'
    if 'conv1x1_split_kernel' in k:  # K20 (before the generic 'conv' match): the f32 1x1 conv on the bf16 matrix cores
        return 'K20'
    if 'conv1x1_16_kernel' in k or 'conv1x1_16_deepk_kernel' in k:  # K13h: the 16-bit 1x1 conv + epilogue
        return 'K13h'
    if any(n in k for n in ('conv1x1_kernel', 'conv1x1_deepk_kernel', 'conv1x1_stream_kernel', 'conv1x1_deep64_kernel')):  # K13 (before the 'conv' / 'gemm' matches): the whole 1x1 conv + epilogue
        return 'K13'
    if 'bias_act' in k:
        return 'K10'
    if 'depthwise5x5' in k:
        return 'K15'
    if 'depthwise3x3_blocks' in k:  # K18 (before K11's match): the stride-1 layers on register blocks
        return 'K18'
    if 'depthwise3x3' in k:
        return 'K11'
    if 'depthwise' in k:  # PyTorch's own depthwise kernel (conv_depthwise2d_forward_kernel)
        return 'dw conv'
    if k.startswith('cijk') or 'gemm' in k:
        return 'gemm'
    if 'sigmoid' in k:
        return 'sigmoid'
    if 'silu' in k:
        return 'silu'
    if 'mul' in k or 'binaryfunctor' in k:
        return 'binary'
    if 'copy_kernel' in k:  # dtype casts (autocast's per-forward weight casts, .to(dtype))
        return 'cast/copy'
    if 'miopen' in k or 'conv' in k:
        return 'conv'
    return 'other'


def _role(module, kind):
    """Role of a kernel inside its MBConv block from the module that launched it and its kind."""
    parts = module.split('.')
    last = parts[-1]
    if kind in ('K10', 'K11', 'K18', 'se_gate'):
        return kind
    if last == 'fc1':
        return 'SE fc1' if kind == 'gemm' else 'SE fc1 bias'
    if last == 'fc2':
        return 'SE fc2' if kind == 'gemm' else 'SE fc2 bias'
    if last == 'act':
        return 'SE act'
    if last == 'gate':
        return 'SE gate fn' if kind == 'sigmoid' else 'x * gate'
    if kind == 'binary':
        return 'x * gate'
    return None


def _fused_table(per_kernel, pat):
    """The FusedMBConv stages (1 - 3) and the stem: per block the dense 3x3 convolution (MIOpen's kernels, layout
    transposes and casts included, or K14h), the K10 pass behind it and the 1x1 project with its epilogue; K16h (the
    whole block as one launch, `record --fuse-blocks`) is launched by the block itself and has its own column."""
    block_pat = re.compile(r'^1\.(\d+)\.(\d+)$')
    rows = OrderedDict()
    served = defaultdict(float)   # what serves the dense convolutions: kernel name (shortened) -> us
    for module, kind, kname, us in per_kernel:
        m = pat.match(module)
        mb = block_pat.match(module) if kind == 'K16h' else None
        if mb:
            rows.setdefault(f'{mb.group(1)}.{mb.group(2)}', defaultdict(float))['K16h'] += us
            continue
        if m and int(m.group(1)) < 4:
            key, layer = f'{m.group(1)}.{m.group(2)}', int(m.group(3))
        elif module.startswith('1.0.') or module == '1.0':
            key, layer = 'stem', 0
        else:
            continue
        b = rows.setdefault(key, defaultdict(float))
        if layer == 0:
            col = kind if kind in ('K14h', 'K19', 'K21', 'K22', 'K10') else 'dense conv'
            if col == 'dense conv' and key != 'stem':
                served[f'{kind}: {kname[:60]}'] += us
        else:
            col = 'project'   # (K13 / K13h / K20, or the library GEMM + K10)
        b[col] += us
    cols = ['dense conv', 'K14h', 'K19', 'K21', 'K22', 'K10', 'project', 'K16h']
    lines = ['', '## FusedMBConv stages and the stem: the dense 3x3 layer, the K10 pass behind it, the 1x1 project '
                 '(or K16h: all of them in one launch)', '',
             '| stage.block | ' + ' | '.join(cols) + ' | **3x3 + K10** |', '|---|' + '---|' * (len(cols) + 1)]
    sums = defaultdict(float)
    for key, b in rows.items():
        dense = b['dense conv'] + b['K14h'] + b['K19'] + b['K21'] + b['K22'] + b['K10']
        for c in cols:
            sums[c] += b[c]
        sums['dense'] += dense
        if key != 'stem':
            sums['dense_blocks'] += dense
        lines.append(f'| {key} | ' + ' | '.join(f'{b[c]:.1f}' for c in cols) + f' | **{dense:.1f}** |')
    lines.append('| **sum** | ' + ' | '.join(f'{sums[c]:.1f}' for c in cols) + f' | **{sums["dense"]:.1f}** |')
    lines += ['', f'Dense 3x3 layers of stages 1 - 3 with their epilogue (without the stem): '
                  f'**{sums["dense_blocks"]:.1f} us**.']
    slice23 = sum(b['dense conv'] + b['K14h'] + b['K19'] + b['K21'] + b['K22'] + b['K10'] + b['project'] + b['K16h']
                  for key, b in rows.items() if key.split('.')[0] in ('2', '3'))
    lines += ['', f'Dense 3x3 + project of stages 2 - 3 (K16h included): **{slice23:.1f} us**.']
    if served:
        lines += ['', 'Library kernels behind the "dense conv" column of stages 1 - 3 (kind: kernel, us):', '']
        lines += [f'- `{k}` {v:.1f}' for k, v in sorted(served.items(), key=lambda kv: -kv[1])[:8]]
    return lines


def _depthwise_table(per_kernel, depthwise, total):
    """Every depthwise layer: k, C, input map, stride, then what served it -- PyTorch's depthwise kernel (or MIOpen)
    + K10, or the one-pass K11 / K18 / K15."""
    if not depthwise:
        return []
    cols = ['conv', 'K10', 'K11', 'K18', 'K15', 'other']
    rows = OrderedDict((n, defaultdict(float)) for n in depthwise)
    for module, kind, kname, us in per_kernel:
        for n in depthwise:
            if module == n or module.startswith(n + '.'):
                col = kind if kind in ('K10', 'K11', 'K18', 'K15') else 'conv' if kind in ('dw conv', 'conv') else 'other'
                rows[n][col] += us
                break
    lines = ['', '## Depthwise layers', '',
             '| layer | k | C | map | stride | ' + ' | '.join(cols) + ' | **sum** |', '|---|---|---|---|---|' + '---|' * (len(cols) + 1)]
    by_k = defaultdict(float)
    for n, b in rows.items():
        k, C, hw, stride = depthwise[n]
        t = sum(b.values())
        by_k[k] += t
        lines.append(f'| {n} | {k} | {C} | {hw} | {stride} | ' + ' | '.join(f'{b[c]:.1f}' for c in cols) + f' | **{t:.1f}** |')
    lines += ['', ' '.join(f'{k}x{k} layers: **{v:.1f} us** ({100 * v / total:.1f} % of the forward\'s {total:.1f} us).'
                           for k, v in sorted(by_k.items()))]
    return lines


def report(args):
    meta = json.load(open(args.markers))
    order = meta['order']
    rows = _kernels(args.trace)
    marks = [i for i, r in enumerate(rows) if MARK in r[2]]
    # the marked forward is the last run of len(order) consecutive markers
    if len(marks) < len(order):
        raise SystemExit(f'{len(marks)} markers in the trace, {len(order)} recorded')
    marks = marks[-len(order):]
    per_kernel = []   # (module, kind, kernel name, us)
    for j, mi in enumerate(marks):
        end = marks[j + 1] if j + 1 < len(marks) else len(rows)
        for r in rows[mi + 1:end]:
            per_kernel.append((order[j], _kind(r[2]), r[2], (r[1] - r[0]) / 1e3))
    total = sum(k[3] for k in per_kernel)
    pat = re.compile(r'^1\.(\d+)\.(\d+)\.block\.(\d+)')
    fused = _fused_table(per_kernel, pat)
    blocks = OrderedDict()
    proj = defaultdict(list)
    convs = meta['conv1x1']
    for module, kind, kname, us in per_kernel:
        m = pat.match(module)
        if not m:
            continue
        stage, idx, layer = int(m.group(1)), int(m.group(2)), int(m.group(3))
        if stage < 4:
            continue  # FusedMBConv stages: no squeeze-excite
        key = (stage, idx)
        b = blocks.setdefault(key, defaultdict(float))
        role = _role(module, kind)
        if role == 'K10' and layer != 3:
            role = None  # the expand layer's epilogue: not part of the tail
        if role is None:
            # the MBConv layers: '0' expand 1x1, '1' depthwise, '2' SE, '3' project
            role = {0: 'expand', 1: 'depthwise', 2: 'SE other', 3: 'project'}.get(layer, f'layer {layer}')
            if role == 'project' and kind in ('gemm', 'conv', 'K13', 'K13h', 'K20'):
                # (K13 runs inside the ConvBiasAct, the library GEMM inside its .conv)
                proj[tuple(convs.get(module) or convs.get(module + '.conv', ('?',)))].append(us)
            # (a layer on K20, `record --split-gemm`, gets its own column: 'expand K20', 'project K20')
            role = role if kind in ('gemm', 'conv', 'K11', 'K18', 'K13', 'K13h') else f'{role} {kind}'
        b[role] += us
    tail_roles = ['SE fc1', 'SE fc1 bias', 'SE act', 'SE fc2', 'SE fc2 bias', 'SE gate fn', 'se_gate', 'x * gate',
                  'project', 'project K20', 'K10']
    roles = [r for r in tail_roles if any(r in b for b in blocks.values())]
    others = sorted({r for b in blocks.values() for r in b} - set(roles))
    lines = [f'# Backbone per-layer kernel times: {meta.get("backbone", "effnetv2-s")}, batch {meta["batch"]}, '
             f'{meta["res"]} px, {meta.get("precision", "f32")}',
             '', f'{args.title}', '',
             f'One marked forward (tools/backbone_trace.py): {len(per_kernel)} kernels, {total:.1f} us of kernel '
             f'time (markers excluded).  Times in us.  "tail" = the squeeze-excite roles + x * gate + project + '
             f'K10 (where a kernel is attributed to "K11" it is the depthwise layer, not the tail).', '',
             '| stage.block | ' + ' | '.join(roles) + ' | **tail** | ' + ' | '.join(others) + ' |',
             '|---|' + '---|' * (len(roles) + 1 + len(others))]
    sums = defaultdict(float)
    for (stage, idx), b in blocks.items():
        tail = sum(b.get(r, 0.0) for r in roles)
        for r in roles + others:
            sums[r] += b.get(r, 0.0)
        sums['tail'] += tail
        lines.append(f'| {stage}.{idx} | ' + ' | '.join(f'{b.get(r, 0.0):.1f}' for r in roles)
                     + f' | **{tail:.1f}** | ' + ' | '.join(f'{b.get(r, 0.0):.1f}' for r in others) + ' |')
    lines.append('| **sum** | ' + ' | '.join(f'{sums[r]:.1f}' for r in roles) + f' | **{sums["tail"]:.1f}** | '
                 + ' | '.join(f'{sums[r]:.1f}' for r in others) + ' |')
    se_chain = sum(sums[r] for r in roles if r.startswith('SE') or r in ('se_gate', 'x * gate'))
    lines += ['', f'Squeeze-excite chain incl. x * gate, stages 4-6: **{se_chain:.1f} us**; '
                  f'whole tail: **{sums["tail"]:.1f} us**; whole forward: {total:.1f} us.', '',
              '## Project GEMMs by shape (Cin -> Cout)', '', '| Cin -> Cout | calls | avg us | sum us |', '|---|---|---|---|']
    for shape, v in sorted(proj.items()):
        lines.append(f'| {" -> ".join(map(str, shape))} | {len(v)} | {sum(v) / len(v):.1f} | {sum(v):.1f} |')
    lines += fused
    if not blocks:   # not an EfficientNetV2 module tree: the block tables above are empty
        lines = lines[:4] + [f'One marked forward (tools/backbone_trace.py): {len(per_kernel)} kernels, {total:.1f} us of '
                             f'kernel time (markers excluded).  Times in us.  (The per-block tables are written for '
                             f'EfficientNetV2 and left out for this backbone.)']
    lines += _depthwise_table(per_kernel, meta.get('depthwise', {}), total)
    kinds = defaultdict(float)
    for _, kind, _, us in per_kernel:
        kinds[kind] += us
    lines += ['', '## Whole forward by kernel kind', '', '| kind | us |', '|---|---|']
    lines += [f'| {k} | {v:.1f} |' for k, v in sorted(kinds.items(), key=lambda kv: -kv[1])]
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines[:8] + lines[-30:]))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest='cmd', required=True)
    r = sub.add_parser('record')
    r.add_argument('--markers', required=True)
    r.add_argument('--batch', type=int, default=64)
    r.add_argument('--res', type=int, default=256)
    r.add_argument('--warmup', type=int, default=3)
    r.add_argument('--backbone', default='effnetv2-s')
    r.add_argument('--fuse-blocks', action='store_true',
                   help='fold with fuse_blocks=True (a -copy precision only): the armed FusedMBConv blocks on K16h')
    r.add_argument('--fuse-stem', action='store_true',
                   help='fold with fuse_stem=True: Preproc + the stem convolution + its epilogue on K17')
    r.add_argument('--block-depthwise', action='store_true',
                   help='fold with block_depthwise=True: the stride-1 depthwise 3x3 layers on K18 where K11 would take '
                        'its generic kernel')
    r.add_argument('--winograd3x3', action='store_true',
                   help='fold with winograd3x3=True (f32 only): the dense 3x3 stride-1 layers on K19')
    r.add_argument('--strided3x3', action='store_true',
                   help='fold with strided3x3=True (f32 only): the dense 3x3 stride-2 layers (Cin a multiple of 4) on K22')
    r.add_argument('--split3x3', action='store_true',
                   help='fold with split3x3=True (f32 only): the dense 3x3 stride-1 layers (Cin a multiple of 8) on K21, '
                        'the split-operand kernel')
    r.add_argument('--split-gemm', action='store_true',
                   help='fold with split_gemm=True (f32 only): the 1x1 stride-1 layers on K20, the split-operand kernel')
    r.add_argument('--deep-projects', action='store_true',
                   help='fold with deep_projects=True (a -copy precision only): the deep project convolutions on '
                        "K13h's deep-K configuration")
    r.add_argument('--no-k13-pre', action='store_true',
                   help='FusedMBConv.use_k13_pre = False: the f32 copy keeps the K10 pass behind the dense 3x3 layers of '
                        'stages 2 - 3 instead of leaving it to the project (K13 with the input prologue)')
    r.add_argument('--no-k15', action='store_true',
                   help='fold with DepthwiseBiasAct.kernel_sizes = (3,): 5x5 depthwise layers on DepthwiseConv2d + K10')
    r.add_argument('--precision', default='f32',
                   choices=['f32', 'f16-autocast', 'bf16-autocast', 'f16-copy', 'bf16-copy'])
    p = sub.add_parser('report')
    p.add_argument('--trace', required=True)
    p.add_argument('--markers', required=True)
    p.add_argument('--out', required=True)
    p.add_argument('--title', default='')
    args = ap.parse_args()
    (record if args.cmd == 'record' else report)(args)


if __name__ == '__main__':
    main()
