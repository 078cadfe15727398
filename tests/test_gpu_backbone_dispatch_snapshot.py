"""GPU: which path every folded layer takes, as a recorded snapshot.  One forward per case; the list of `last_path` over
the modules that have one, in module order, must equal tests/golden/backbone_dispatch_paths.json -- our own result,
recorded on the MI355X by record() below (PYTHONPATH=. python tests/test_gpu_backbone_dispatch_snapshot.py OUT.json).
The paths depend on shapes, dtypes, the call's mode and the shipped `*_slower` lists, never on values: the weights are
oracle.cases.deterministic_state, uncalibrated.  A pull request that adds a kernel or moves a layer to another one
records the file again, and its diff names every layer that moved."""
import contextlib
import functools
import json
import os

import pytest
import torch

from test_backbone_option_combos_host import F32_OPTS, H16_OPTS
from test_gpu_conv1x1_split import _pinned

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'backbone_dispatch_paths.json')
DTYPES = {'f32': None, 'f16': torch.float16, 'bf16': torch.bfloat16}
# (network, crop side, batch).  EfficientNetV2-S at 192 px ends in 6x6 maps, where the 1x1 kernels refuse
SETS = [('efficientnetv2-s', 256, 2), ('efficientnetv2-s', 192, 2), ('mobilenetv3', 256, 1), ('resnet18', 128, 1)]
CASES = [(name, res, batch, dt, copy) for name, res, batch in SETS for dt in DTYPES for copy in ('default', 'all_on')]
# calls the kernels refuse (K17 alone reads channels_last crops): EfficientNetV2-S at 128 px, batch 1, all-on copies
REFUSALS = [(dt, why) for dt in ('f32', 'f16') for why in ('autocast', 'grad', 'channels_last')]


def case_id(name, res, batch, dt, copy, why=None):
    return f'{name}-{res}px-b{batch}-{dt}-{copy}' + ('' if why is None else '-' + why)


@functools.lru_cache(maxsize=None)
def _net(name):
    from metrabs_amd import backbones
    from oracle import cases
    net = backbones.build_backbone(name)
    net.load_state_dict(cases.deterministic_state(net.state_dict()))
    return net.eval().cuda()


@functools.lru_cache(maxsize=None)
def folded_copy(name, dt, copy):
    """The folded copy of one case: made once, shared, its weights never written."""
    from metrabs_amd import backbones
    opts = () if copy == 'default' else (F32_OPTS if dt == 'f32' else H16_OPTS)
    return backbones.fold_batchnorm(_net(name), fused_epilogue=True, dtype=DTYPES[dt], **{o: True for o in opts})


def case_input(res, batch):
    return torch.rand(batch, 3, res, res, generator=torch.Generator().manual_seed(res + batch)).cuda()


def paths_of(net):
    return [m.last_path for m in net.modules() if hasattr(m, 'last_path')]


def run_case(name, res, batch, dt, copy, why=None):
    """-> (features, paths) of one forward.  why: None (inference_mode), 'autocast', 'grad' (grad mode, the copy's
    parameters requiring grad) or 'channels_last'."""
    net, x = folded_copy(name, dt, copy), case_input(res, batch)
    for m in net.modules():
        if hasattr(m, 'last_path'):
            m.last_path = None
    if why == 'channels_last':
        x = x.contiguous(memory_format=torch.channels_last)
    params = [p for p in net.parameters() if p.is_floating_point()]
    was = [p.requires_grad for p in params]
    with contextlib.ExitStack() as stack:
        stack.enter_context(_pinned())
        if why == 'grad':
            for p in params:
                p.requires_grad_(True)
        else:
            stack.enter_context(torch.inference_mode())
        if why == 'autocast':
            stack.enter_context(torch.autocast('cuda', torch.float16))
        try:
            y = net(x).detach().clone()
        finally:
            for p, r in zip(params, was):
                p.requires_grad_(r)
    return y, paths_of(net)


def record(out=None):
    """Runs every case and writes {case id: paths} (one case per line) to `out`, or prints it."""
    got = {case_id(*c): run_case(*c)[1] for c in CASES}
    for dt, why in REFUSALS:
        c = ('efficientnetv2-s', 128, 1, dt, 'all_on', why)
        got[case_id(*c)] = run_case(*c)[1]
    lines = [f'{json.dumps(k)}: {json.dumps(v, separators=(",", ":"))}' for k, v in got.items()]
    text = '{\n' + ',\n'.join(lines) + '\n}\n'
    if out is None:
        print(text, end='')
    else:
        with open(out, 'w') as f:
            f.write(text)


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def _check(case):
    y, paths = run_case(*case)
    want = _recorded()[case_id(*case)]
    if len(case) == 5:
        assert y.dtype == (DTYPES[case[3]] or torch.float32)
    assert len(paths) == len(want)
    moved = [(i, w, p) for i, (w, p) in enumerate(zip(want, paths)) if w != p]
    assert not moved, (len(moved), moved[:8])
    return paths


@pytest.mark.parametrize('name,res,batch,dt,copy', CASES, ids=[case_id(*c) for c in CASES])
def test_every_layer_takes_the_recorded_path(name, res, batch, dt, copy, hip_lib):
    _check((name, res, batch, dt, copy))


@pytest.mark.parametrize('dt,why', REFUSALS, ids=[f'{d}-{w}' for d, w in REFUSALS])
def test_refused_calls_take_the_recorded_path(dt, why, hip_lib):
    _check(('efficientnetv2-s', 128, 1, dt, 'all_on', why))


if __name__ == '__main__':
    import sys
    record(sys.argv[1] if len(sys.argv) > 1 else None)
