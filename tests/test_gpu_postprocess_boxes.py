"""GPU: K7 (metrabs_amd/csrc/postprocess.hip) where tests/test_gpu_postprocess.py cannot fail -- there every box of a
call shares one extrinsic matrix and one distortion vector, the mirror mapping is the identity unless J = 17, and
nothing looks at memory next to the outputs, at repeats, or at the entry's refusals.

Here every box has its own camera (tests/test_posthead_cases_host.py shows on the CPU that the oracle's answer moves
by > 100 bounds when box 0's camera is used for all), boxes with and without distortion share a launch, a box's bits
must not depend on its batch mates, and the TTA mean must be the double sum the kernel says it is.
Bounds against the oracle are those of tests/test_gpu_postprocess.py: 1.5e-3 mm, 2e-3 px, times its `grow`."""
import ctypes

import pytest
import torch

from oracle import cases, cpu_ref
from test_gpu_postprocess import make_inputs

pytestmark = pytest.mark.gpu

BOX_CONFIGS = [
    dict(id='n5_a5_j17', n=5, A=5, J=17, jt=0, skeleton=None),
    dict(id='n3_a4_j17_jt24_skel', n=3, A=4, J=17, jt=24, skeleton=[1, 3, 23, 7]),
    # A * J = 900 > 256 threads: the un-swap loop takes several passes, with a mirror mapping that moves every joint
    dict(id='n4_a3_j300_pairswap', n=4, A=3, J=300, jt=0, skeleton=None, pair_swap=True),
]
GUARD = 64
E_NULL, E_SHAPE = -1, -2   # MTR_E_NULL, MTR_E_SHAPE (include/metrabs_hip.h)


def box_inputs(cfg, seed=None):
    """make_inputs of the existing K7 test, then a camera of its own for every box (cases.per_box_cameras)."""
    seed = 5300 + cfg['n'] + cfg['J'] if seed is None else seed
    poses, rot, flip, mirror, _, _, _, jtm, skel = make_inputs(cfg['n'], cfg['A'], cfg['J'], seed, None, cfg['jt'],
                                                                cfg['skeleton'])
    if cfg.get('pair_swap'):
        mirror = cases.pair_swap_mapping(cfg['J'])
        assert bool(flip.any()) and bool((mirror != torch.arange(cfg['J'])).all())
    K, dist, E = cases.per_box_cameras(cfg['n'], seed + 1)
    return dict(poses=poses, rot=rot, flip=flip, mirror=mirror, K=K, dist=dist, E=E, jtm=jtm, skel=skel,
                A=cfg['A'], n=cfg['n'], J=cfg['J'])


def oracle_boxes(inp, average_aug):
    with torch.inference_mode():
        return cpu_ref.postprocess_from_crop_outputs(inp['poses'], inp['rot'], inp['flip'], inp['mirror'], inp['K'],
                                                     inp['dist'], inp['E'], inp['jtm'], inp['skel'], average_aug)


def box_slice(inp, b):
    """The inputs of a 1-box call holding box b of `inp`."""
    A, n, J = inp['A'], inp['n'], inp['J']
    return dict(inp, poses=inp['poses'].reshape(A, n, J, 3)[:, b:b + 1].reshape(A, J, 3).contiguous(),
                rot=inp['rot'][:, b:b + 1].contiguous(), K=inp['K'][b:b + 1], dist=inp['dist'][b:b + 1],
                E=inp['E'][b:b + 1], n=1)


def run_k7(inp, average_aug):
    from metrabs_amd import kernels
    c = lambda t: None if t is None else t.cuda()
    return kernels.postprocess_poses(inp['poses'].cuda(), inp['rot'].cuda(), inp['flip'], inp['mirror'], inp['K'].cuda(),
                                     inp['dist'].cuda(), torch.linalg.inv(inp['E']).cuda(), c(inp['jtm']), c(inp['skel']),
                                     average_aug)


class RawCall:
    """mtr_postprocess_poses through ctypes on device tensors the test owns: outputs inside guarded buffers, chosen
    pointers NULL, chosen sizes."""

    def __init__(self, inp, average_aug):
        from metrabs_amd import _lib
        self.lib, self.avg = _lib.load(), average_aug
        A, n, J = inp['A'], inp['n'], inp['J']
        self.A, self.n, self.J = A, n, J
        f = lambda t: t.float().contiguous().cuda()
        self.t = dict(poses=f(inp['poses']), rot=f(inp['rot']), flip=inp['flip'].to(torch.uint8).cuda(),
                      mirror=inp['mirror'].to(torch.int32).cuda(), K=f(inp['K']), dist=f(inp['dist']),
                      invE=f(torch.linalg.inv(inp['E'])),
                      jtm=f(inp['jtm']) if inp['jtm'] is not None else None,
                      skel=inp['skel'].to(torch.int32).cuda() if inp['skel'] is not None else None)
        self.Jt = inp['jtm'].shape[1] if inp['jtm'] is not None else J
        self.S = inp['skel'].numel() if inp['skel'] is not None else self.Jt
        self.rows = n * (self.S if average_aug else A * self.S)
        self.buf3 = torch.full((GUARD + self.rows * 3 + GUARD,), float('nan'), device='cuda')
        self.buf2 = torch.full((GUARD + self.rows * 2 + GUARD,), float('nan'), device='cuda')

    def outs(self):
        return self.buf3[GUARD:GUARD + self.rows * 3], self.buf2[GUARD:GUARD + self.rows * 2]

    def guards_are_nan(self):
        return all(bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[len(b) - GUARD:]).all())
                   for b in (self.buf3, self.buf2))

    def call(self, null=None, **over):
        from metrabs_amd._lib import current_stream_ptr
        t = self.t
        p = lambda k: None if (k == null or t.get(k) is None) else ctypes.c_void_p(t[k].data_ptr())
        o3, o2 = self.outs()
        a = dict(A=self.A, n=self.n, J=self.J, Jt=self.Jt, S=self.S)
        a.update(over)
        return self.lib.mtr_postprocess_poses(
            p('poses'), p('rot'), p('flip'), p('mirror'), p('jtm'), a['Jt'], p('skel'), a['S'], p('K'), p('dist'),
            p('invE'), a['A'], a['n'], a['J'], int(self.avg),
            None if null == 'out3' else ctypes.c_void_p(o3.data_ptr()),
            None if null == 'out2' else ctypes.c_void_p(o2.data_ptr()), current_stream_ptr(o3.device))


@pytest.mark.parametrize('avg', [True, False])
@pytest.mark.parametrize('cfg', BOX_CONFIGS, ids=[c['id'] for c in BOX_CONFIGS])
def test_every_box_uses_its_own_camera(cfg, avg, hip_lib):
    """Per-box extrinsics, intrinsics and distortion; boxes without, with 5 and with 12 coefficients in one launch
    (has_dist is decided per box inside the kernel)."""
    inp = box_inputs(cfg)
    o3, o2 = oracle_boxes(inp, avg)
    p3, p2 = run_k7(inp, avg)
    assert p3.shape == o3.shape and p2.shape == o2.shape
    e3, e2 = float((p3.cpu() - o3).abs().max()), float((p2.cpu() - o2).abs().max())
    print(f'[parity] postprocess per-box cameras {cfg["id"]} avg={avg}: poses3d max {e3:.2e} mm, poses2d max {e2:.2e} px')
    grow = max(1.0, cfg['J'] / 122) if cfg['jt'] else 1.0
    assert e3 <= 1.5e-3 * grow and e2 <= 2e-3 * grow


@pytest.mark.parametrize('avg', [True, False])
@pytest.mark.parametrize('cfg', BOX_CONFIGS[:2], ids=[c['id'] for c in BOX_CONFIGS[:2]])
def test_a_box_does_not_depend_on_its_batch_mates(cfg, avg, hip_lib):
    """Box b of an n-box call == the 1-box call on box b's slices, bit for bit (the [A][n][J][3] input stride and the
    output offset change with n; the arithmetic does not)."""
    inp = box_inputs(cfg)
    p3, p2 = run_k7(inp, avg)
    for b in (0, cfg['n'] // 2, cfg['n'] - 1):
        s3, s2 = run_k7(box_slice(inp, b), avg)
        assert torch.equal(s3[0], p3[b]) and torch.equal(s2[0], p2[b]), b


@pytest.mark.parametrize('A', [1, 3, 5, 10])
def test_tta_mean_is_the_double_sum_of_the_per_aug_outputs(A, hip_lib):
    """average_aug=True == float32(double(sum over a = 0 .. A-1 of the average_aug=False outputs, in that order) *
    double(1.0 / A)): what the kernel's last lines state, bit for bit."""
    inp = box_inputs(dict(n=4, A=A, J=17, jt=0, skeleton=None), seed=5400 + A)
    per3, per2 = run_k7(inp, False)
    avg3, avg2 = run_k7(inp, True)
    for per, avg in ((per3, avg3), (per2, avg2)):
        s = torch.zeros_like(avg, dtype=torch.float64)
        for a in range(A):
            s = s + per[:, a].double()
        assert torch.equal((s * (1.0 / A)).float(), avg)


@pytest.mark.parametrize('cfg', [BOX_CONFIGS[1], BOX_CONFIGS[2]], ids=[BOX_CONFIGS[1]['id'], BOX_CONFIGS[2]['id']])
def test_memory_repeats_and_graph_replay(cfg, hip_lib):
    """NaN-filled outputs inside 64-element guard bands: every element written, the bands untouched, the inputs
    unchanged; three calls and three replays of a captured graph give the first call's bits."""
    inp = box_inputs(cfg)
    for avg in (True, False):
        r = RawCall(inp, avg)
        before = {k: v.clone() for k, v in r.t.items() if v is not None}
        assert r.call() == 0
        torch.cuda.synchronize()
        first = [o.clone() for o in r.outs()]
        assert not any(bool(torch.isnan(o).any()) for o in first) and r.guards_are_nan()
        assert all(torch.equal(v, r.t[k]) for k, v in before.items())
        want3, want2 = run_k7(inp, avg)
        assert torch.equal(first[0], want3.flatten()) and torch.equal(first[1], want2.flatten())
        for _ in range(2):
            for o in r.outs():
                o.fill_(float('nan'))
            assert r.call() == 0
            assert all(torch.equal(a, b) for a, b in zip(r.outs(), first)) and r.guards_are_nan()
        # (captured under inference mode like every capture of this project: torch updates the generator's graph-state
        #  tensors in place at capture_begin, and another test's capture may have made them inference tensors)
        with torch.inference_mode():
            stream = torch.cuda.Stream()
            stream.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(stream):
                with torch.cuda.graph(graph, stream=stream, capture_error_mode='thread_local'):
                    assert r.call() == 0
            torch.cuda.current_stream().wait_stream(stream)
        for _ in range(3):
            for o in r.outs():
                o.fill_(float('nan'))
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(r.outs(), first)) and r.guards_are_nan()


def test_no_boxes_touches_nothing(hip_lib):
    r = RawCall(box_inputs(BOX_CONFIGS[0]), True)
    assert r.call(n=0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(r.buf3).all()) and bool(torch.isnan(r.buf2).all())


def test_more_than_48_kib_of_lds_twice_in_one_process(hip_lib):
    """A = 5, J = 555: 66 600 bytes of LDS, through allow_dynamic_lds -- on a first and on a second call."""
    cfg = dict(id='lds', n=3, A=5, J=555, jt=0, skeleton=list(range(0, 555, 7)))
    inp = box_inputs(cfg)
    o3, o2 = oracle_boxes(inp, True)
    outs = [run_k7(inp, True) for _ in range(2)]
    for p3, p2 in outs:
        assert float((p3.cpu() - o3).abs().max()) <= 1.5e-3 and float((p2.cpu() - o2).abs().max()) <= 2e-3
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_the_lds_limit_is_pinned_on_both_sides(hip_lib):
    """A * J = 6144 (144 KiB of LDS) runs and matches the oracle; 6145 is MTR_E_SHAPE with no launch."""
    cfg = dict(id='limit', n=2, A=3, J=2048, jt=0, skeleton=None, pair_swap=True)
    inp = box_inputs(cfg)
    o3, o2 = oracle_boxes(inp, False)
    p3, p2 = run_k7(inp, False)
    e3, e2 = float((p3.cpu() - o3).abs().max()), float((p2.cpu() - o2).abs().max())
    print(f'[parity] postprocess A*J = 6144: poses3d max {e3:.2e} mm, poses2d max {e2:.2e} px')
    assert e3 <= 1.5e-3 and e2 <= 2e-3
    r = RawCall(box_inputs(dict(id='x', n=1, A=1, J=17, jt=0, skeleton=None)), True)
    # (shape checks come before any read: the tensors behind the pointers are those of the 17-joint call)
    assert r.call(A=1, J=6145) == E_SHAPE and r.call(A=5, J=1229) == E_SHAPE
    torch.cuda.synchronize()
    assert bool(torch.isnan(r.buf3).all())


def test_refusals(hip_lib):
    r = RawCall(box_inputs(BOX_CONFIGS[1]), True)
    assert r.call(Jt=0) == E_SHAPE and r.call(Jt=-3) == E_SHAPE   # a joint transform with no columns
    assert r.call(S=0) == E_SHAPE                                           # an empty skeleton
    assert r.call(A=0) == E_SHAPE and r.call(J=0) == E_SHAPE and r.call(n=-1) == E_SHAPE
    for k in ('poses', 'rot', 'flip', 'mirror', 'K', 'dist', 'invE', 'out3', 'out2'):
        assert r.call(null=k) == E_NULL, k
    torch.cuda.synchronize()
    assert bool(torch.isnan(r.buf3).all()) and bool(torch.isnan(r.buf2).all())
    assert r.call() == 0 and not bool(torch.isnan(r.outs()[0]).any())
