"""GPU: K5 (metrabs_amd/csrc/reconstruct.hip) on the paths the parity cases do not reach.

mtr_reconstruct_absolute takes ONE launch while B * J <= 16384 and moments -> finalize -> solve above that; the largest
B * J elsewhere in the suite is 12 371, so the second branch (the one an internal batch of 64 crops of a 555-point head
takes), its workspace handling, the grid-stride loop of the moments kernel (> 1024 crops) and the lane-stride loop of
the finalize kernel (> 64 partial rows) run here for the first time -- at shapes just over the limit, and at 128 x 128
= 16 384, the last shape of the one-launch kernel.

The bound against float64 (cpu_ref.reconstruct_absolute on .double() inputs; every element is checked):

    |K5 - fp64| <= 2 ulp32(M_joint) + 0.5 ulp32(max(M_joint, M_ref))        (cases.recon_ulp_bound)

with M_joint the joint's largest absolute coordinate and M_ref the largest absolute coordinate of its crop's reference
point: 2.5 ulp of float32 at the joint (1.2e-3 mm at 4 - 8 m) wherever the reference point is no larger than the joint.
Derivation: K5 sums in float64 and rounds to float32 four times, half an ulp each -- (1) the reference point, (2) rel +
ref, (3) the normalized coordinate (times the depth: half an ulp of the back-projected coordinate), (4) the final store
-- plus 0.5 ulp for the order of the float64 sums (fp64 normal equations here, fp64 lstsq in the reference; the
weights 1e-4 of out-of-FOV joints leave the systems well conditioned against the ridge 1e-2).
Which rounding a flat "2.5 ulp at the joint" misses: (1) happens at the magnitude of the REFERENCE POINT, not of the
joint.  Where rel + ref cancels the joint is smaller than its reference point and half an ulp of ref is more than half
an ulp of the joint: a crop of the 4097 x 4 case with a single joint in the FOV (3 % of its crops) is pulled to the
origin by the ridge, ref ~ -rel, |ref| = 124 mm, the joint 4 mm from the origin -- the CPU emulation of K5's arithmetic
(tests/test_posthead_cases_host.py) measures 3.6 ulp of the joint there, 1.5 ulp at every other shape and 1.0 ulp over
the joints that are no smaller than their reference point.  So term (1) is counted where it happens.

The moments are compared with float64 sums directly (no output-level test can see a wrong moment sum: the two RMS
scales enter the solution through the ridge term only), crops must not depend on their batch mates bit for bit, and
the memory around the output, repeats, graph replay and the entries' refusals are checked on both paths."""
import ctypes
import functools

import pytest
import torch

from oracle import cases, cpu_ref

pytestmark = pytest.mark.gpu

GUARD = 64
E_NULL, E_SHAPE, E_PARAM, E_WORKSPACE = -1, -2, -4, -5   # include/metrabs_hip.h
LIMIT = 16384                                             # kFusedMaxElems: B * J of the one-launch kernel

SHAPES = dict(cases.RECON_PATH_SHAPES, general_k=cases.RECON_GENERAL_K_SHAPE)


def mcfg(cfg):
    from metrabs_amd.config import MetrabsConfig
    return MetrabsConfig.from_any(cfg.as_dict())


@functools.lru_cache(maxsize=None)
def shape_case(name):
    """(inputs, the float64 pieces) of a shape, computed once and left unchanged."""
    B, J = SHAPES[name]
    c2d, rel, K, cfg, _ = cases.recon_paths_case(B, J, 8700 + J, general_k=(name == 'general_k'))
    return (c2d, rel, K, cfg), cases.recon_candidates_fp64(c2d, rel, K, cfg)


def ulp_figures(out, c):
    """(max error in ulp32 at the joint over the joints no smaller than their reference point: the flat 2.5 ulp; the
    same over the other joints; max error / bound over every element)"""
    want = c['out']
    err = (out.double() - want).abs()
    ulp = cases.f32_ulp_at(want.abs().amax(dim=-1, keepdim=True))
    bound = cases.recon_ulp_bound(want, c['ref'])
    plain = (bound <= 2.5 * ulp).expand_as(err)
    rest = (err / ulp)[~plain]
    return float((err / ulp)[plain].max()), float(rest.max()) if rest.numel() else 0.0, float((err / bound).max())


def moments_fp64(c2d, rel, K):
    """(sum normalized2d^2, sum rel_backproj^2, count) as float64 torch sums, from torch.linalg.inv(K.double())."""
    inv = torch.linalg.inv(K.double())
    n = (cpu_ref.to_homogeneous(c2d.double()) @ inv.transpose(1, 2))[..., :2]
    rb = n * rel.double()[..., 2:] - rel.double()[..., :2]
    return torch.stack([n.square().sum(), rb.square().sum(), torch.tensor(2.0 * c2d.shape[0] * c2d.shape[1]).double()])


@pytest.mark.parametrize('name', list(SHAPES))
def test_output_vs_fp64_either_side_of_the_one_launch_limit(name, hip_lib):
    """Every element within the module's bound of the float64 evaluation, and the project's bounds against the float32
    LAPACK oracle (MPJPE 1e-3 mm, max 4e-3 mm) beside it.  general_k: skew, K[1,0] and a bottom row [g, h, 1]."""
    from metrabs_amd import kernels
    (c2d, rel, K, cfg), c = shape_case(name)
    B, J = SHAPES[name]
    assert (B * J > LIMIT) == (name != 'b128_j128') and B * J - LIMIT <= 116
    out = kernels.reconstruct_absolute(c2d.cuda(), rel.cuda(), K.cuda(), mcfg(cfg)).cpu()
    ulps, ulps_small, worst = ulp_figures(out, c)
    with torch.inference_mode():
        oracle = cpu_ref.reconstruct_absolute(c2d, rel, K, cfg)
    e_mean, e_max = cpu_ref.mpjpe(out, oracle), float((out - oracle).abs().max())
    print(f'[parity] K5 {name} ({B} x {J}, {"two launches" if B * J > LIMIT else "one launch"}): max {ulps:.2f} ulp vs fp64 '
          f'({ulps_small:.2f} ulp over joints smaller than their reference point, {worst:.2f} of the bound, '
          f'{float((out.double() - c["out"]).abs().max()):.2e} mm); vs the f32 oracle MPJPE {e_mean:.2e} max {e_max:.2e} mm')
    assert worst <= 1.0 and ulps <= 2.5
    assert e_mean <= 1e-3 and e_max <= 4e-3


@pytest.mark.parametrize('B,scaled', [(B, s) for B in (1030, 257, 256, 5, 1, 0) for s in (None, 'first', 'last') if B or s is None])
def test_moments_are_the_fp64_sums(B, scaled, hip_lib):
    """kernels.reconstruct_moments against float64 torch sums, relative 1e-10: four orders above the float64 summation
    error of 33 k terms (n 2^-53 = 4e-12), seven orders below one missing crop's share (1 / B = 1e-3).  B = 1030: the
    grid-stride loop of the 256-block moments kernel and 258 partial rows (> 64 lanes of the finalize kernel); 257 and
    256: 65 and 64 partial rows.  A second and third run with crop 0 / the last crop scaled by 10: that crop then
    holds most of the sum."""
    from metrabs_amd import kernels
    J = 16
    c2d, rel, K, _, _ = cases.recon_paths_case(B, J, 8600 + B)
    if scaled is not None:
        i = 0 if scaled == 'first' else B - 1
        c2d[i] *= 10
        rel[i] *= 10
    got = kernels.reconstruct_moments(c2d.cuda(), rel.cuda(), K.cuda()).cpu()
    want = moments_fp64(c2d, rel, K)
    assert float(got[2]) == 2 * B * J == float(want[2])
    if B == 0:
        assert got.tolist() == [0.0, 0.0, 0.0]
        return
    r = ((got[:2] - want[:2]).abs() / want[:2]).tolist()
    print(f'[parity] K5 moments B={B} scaled={scaled}: relative error {r[0]:.1e} (normalized2d^2), {r[1]:.1e} (rel_backproj^2)')
    assert max(r) <= 1e-10


def test_solve_does_not_depend_on_batch_mates(hip_lib):
    """reconstruct_solve with FIXED moments: crops [0:1], [5:9], [1024:1030] and [1029:1030] of the 1030-crop call carry
    the bits of the same call on those slices alone."""
    from metrabs_amd import kernels
    (c2d, rel, K, cfg), _ = shape_case('b1030_j16')
    m = mcfg(cfg)
    c2d, rel, K = c2d.cuda(), rel.cuda(), K.cuda()
    moments = kernels.reconstruct_moments(c2d, rel, K)
    full = kernels.reconstruct_solve(c2d, rel, K, moments, m)
    assert torch.equal(full, kernels.reconstruct_absolute(c2d, rel, K, m))   # the monolithic entry: the same two steps
    for s in (slice(0, 1), slice(5, 9), slice(1024, 1030), slice(1029, 1030)):
        part = kernels.reconstruct_solve(c2d[s].contiguous(), rel[s].contiguous(), K[s].contiguous(), moments, m)
        assert torch.equal(part, full[s]), s


def test_weak_perspective_large_path_equals_chunks_on_the_one_launch_path(hip_lib):
    """Weak perspective uses no batch moments: 1030 x 16 through the monolithic entry (solve kernel, 32-byte workspace)
    == the same crops in chunks of 64 (one-launch kernel), bit for bit; and both are the oracle's answer."""
    from metrabs_amd import kernels
    (c2d, rel, K, cfg), _ = shape_case('b1030_j16')
    m = mcfg(cfg)
    g = [t.cuda() for t in (c2d, rel, K)]
    big = kernels.reconstruct_absolute(*g, m, weak_perspective=True,
                                       workspace=torch.empty(4, device='cuda', dtype=torch.float64))
    chunks = torch.cat([kernels.reconstruct_absolute(*(t[i:i + 64].contiguous() for t in g), m, weak_perspective=True)
                        for i in range(0, len(c2d), 64)])
    assert torch.equal(big, chunks)
    want = cases.recon_candidates_fp64(c2d, rel, K, cfg, weak_perspective=True)
    err = (big.cpu().double() - want['out']).abs()
    print(f'[parity] K5 weak perspective 1030 x 16: max {float(err.max()):.2e} mm vs fp64, '
          f'{float((err / cases.recon_ulp_bound(want["out"], want["ref"])).max()):.2f} of the bound')
    assert bool((err <= cases.recon_ulp_bound(want['out'], want['ref'])).all())


def test_shards_of_1000_0_29_and_1_crops(hip_lib):
    """Moments over shards, summed (what an all-reduce does) == the whole-batch moments to relative 1e-12 (only the
    summation order differs); reconstruct_solve per shard with the summed moments within 1e-4 mm of the monolithic
    call (the bound of test_reconstruct_batch_coupling_and_split).  One shard is empty."""
    from metrabs_amd import kernels
    (c2d, rel, K, cfg), _ = shape_case('b1030_j16')
    m = mcfg(cfg)
    g = [t.cuda() for t in (c2d, rel, K)]
    shards = [slice(0, 1000), slice(1000, 1000), slice(1000, 1029), slice(1029, 1030)]
    whole = kernels.reconstruct_moments(*g)
    parts = [kernels.reconstruct_moments(*(t[s].contiguous() for t in g)) for s in shards]
    assert parts[1].tolist() == [0.0, 0.0, 0.0]
    summed = sum(parts)
    rel_err = float(((summed - whole).abs() / whole).max())
    print(f'[parity] K5 moments of 4 shards vs the whole batch: relative {rel_err:.1e}')
    assert rel_err <= 1e-12 and float(summed[2]) == float(whole[2])
    full = kernels.reconstruct_absolute(*g, m)
    # (the empty shard joins the sum and has nothing to solve: an empty tensor has no address for the entry to take,
    #  and Pose3dEstimator does not call the solve for an empty slice either)
    outs = [kernels.reconstruct_solve(*(t[s].contiguous() for t in g), summed, m) for s in shards if s.stop > s.start]
    assert float((torch.cat(outs) - full).abs().max()) <= 1e-4


@pytest.mark.parametrize('centered_stride', [True, False])
def test_fov_edges(centered_stride, hip_lib):
    """Joints exactly on `lower` / `upper` and one float32 step to either side (no mixing): the inside ones carry the
    back-projected value, the outside ones rel + ref -- the candidates lie > 100 bounds apart (CPU test)."""
    from metrabs_amd import kernels
    c2d, rel, K, cfg, lower, upper, expect, n_edge = cases.recon_fov_edges_case(centered_stride)
    c = cases.recon_candidates_fp64(c2d, rel, K, cfg)
    assert cfg.mix_3d_inside_fov is None and torch.equal(c['in_fov'], expect)
    out = kernels.reconstruct_absolute(c2d.cuda(), rel.cuda(), K.cuda(), mcfg(cfg), mix_3d_inside_fov=None).cpu().double()
    bound = cases.recon_ulp_bound(c['out'], c['ref'])
    assert bool(((out - c['out']).abs() <= bound).all())
    inside = expect[:, :n_edge, None]
    near_2d = ((out - c['abs_2d_based']).abs() <= bound)[:, :n_edge].all(-1, keepdim=True)
    near_3d = ((out - c['abs_3d_based']).abs() <= bound)[:, :n_edge].all(-1, keepdim=True)
    assert torch.equal(near_2d, inside) and torch.equal(near_3d, ~inside)


def guarded(B, J):
    buf = torch.full((GUARD + B * J * 3 + GUARD,), float('nan'), device='cuda')
    return buf, buf[GUARD:GUARD + B * J * 3].view(B, J, 3)


def guards_are_nan(buf):
    return bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[len(buf) - GUARD:]).all())


@pytest.mark.parametrize('name', ['b1030_j16', 'b65_j253', 'b128_j128'])
def test_memory_and_repeats(name, hip_lib):
    """The output inside a NaN-filled buffer with 64-element guard bands: every element written (in the FOV or not),
    the bands untouched, the inputs bit-identical afterwards; three calls give identical bits (fixed-order sums, no
    atomics: the file header of reconstruct.hip) -- on both paths."""
    from metrabs_amd import kernels
    (c2d, rel, K, cfg), c = shape_case(name)
    B, J = SHAPES[name]
    assert bool(c['in_fov'].any()) and bool((~c['in_fov']).any())
    g = [t.cuda() for t in (c2d, rel, K)]
    first = None
    for _ in range(3):
        buf, out = guarded(B, J)
        ws = kernels.reconstruct_workspace(B, J, 'cuda')
        ws_buf = torch.full((ws.numel() + 2 * GUARD,), float('nan'), device='cuda', dtype=torch.float64)
        kernels.reconstruct_absolute(*g, mcfg(cfg), workspace=ws_buf[GUARD:GUARD + ws.numel()], out=out)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(out).any()) and guards_are_nan(buf) and guards_are_nan(ws_buf)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(g, (c2d, rel, K)))
        first = out.clone() if first is None else first
        assert torch.equal(out, first)


def test_graph_replay_of_the_large_path(hip_lib):
    """Moments, finalize and solve captured in a torch.cuda.graph replay to the eager bits, three times."""
    from metrabs_amd import kernels
    (c2d, rel, K, cfg), _ = shape_case('b1030_j16')
    B, J = SHAPES['b1030_j16']
    m = mcfg(cfg)
    g = [t.cuda() for t in (c2d, rel, K)]
    eager = kernels.reconstruct_absolute(*g, m)
    ws = kernels.reconstruct_workspace(B, J, 'cuda')
    buf, out = guarded(B, J)
    # (captured under inference mode like every capture of this project: torch updates the generator's graph-state
    #  tensors in place at capture_begin, and another test's capture may have made them inference tensors)
    with torch.inference_mode():
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            kernels.reconstruct_absolute(*g, m, workspace=ws, out=out)   # warm-up on the capture stream
            stream.synchronize()
            with torch.cuda.graph(graph, stream=stream, capture_error_mode='thread_local'):
                kernels.reconstruct_absolute(*g, m, workspace=ws, out=out)
        torch.cuda.current_stream().wait_stream(stream)
    for _ in range(3):
        out.fill_(float('nan'))
        ws.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and guards_are_nan(buf)


def test_entry_rules_without_a_launch(hip_lib):
    """The refusals of the three entries through ctypes; a refused call launches nothing (the poisoned output stays)."""
    from metrabs_amd import kernels
    from metrabs_amd._lib import current_stream_ptr
    (c2d, rel, K, cfg), _ = shape_case('b1030_j16')
    B, J = SHAPES['b1030_j16']
    m = mcfg(cfg)
    g = [t.cuda() for t in (c2d, rel, K)]
    buf, out = guarded(B, J)
    need = hip_lib.mtr_reconstruct_workspace_bytes(B, J)
    assert need == (4 + 2 * 256) * 8
    ws = torch.full((need // 8 + 4,), float('nan'), device='cuda', dtype=torch.float64)
    moments = torch.ones(3, device='cuda', dtype=torch.float64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = current_stream_ptr(out.device)

    def absolute(B=B, J=J, rp=None, ws_ptr=None, ws_bytes=need, **kw):
        rp = m.recon_params(**kw) if rp is None else rp
        return hip_lib.mtr_reconstruct_absolute(p(g[0]), p(g[1]), p(g[2]), B, J, ctypes.byref(rp), p(out),
                                                ctypes.c_void_p(ws.data_ptr() if ws_ptr is None else ws_ptr), ws_bytes, stream)

    def solve(moments_ptr, rp=None, B=B, J=J, **kw):
        rp = m.recon_params(**kw) if rp is None else rp
        return hip_lib.mtr_reconstruct_solve(p(g[0]), p(g[1]), p(g[2]), B, J, ctypes.byref(rp), moments_ptr, p(out), stream)

    assert ws.data_ptr() % 16 == 0
    assert absolute(ws_bytes=need - 1) == E_WORKSPACE                       # one byte short
    assert absolute(ws_ptr=ws.data_ptr() + 8) == E_WORKSPACE                # base not 16-byte aligned
    assert absolute(ws_bytes=24, weak_perspective=True) == E_WORKSPACE     # weak perspective: 32 bytes
    assert solve(None) == E_NULL                                            # full perspective needs the moments
    bad = m.recon_params()
    bad.proc_side = 0
    assert absolute(rp=bad) == E_PARAM and solve(p(moments), rp=bad) == E_PARAM
    assert absolute(J=0) == E_SHAPE and absolute(B=-1) == E_SHAPE
    assert solve(p(moments), J=0) == E_SHAPE and solve(p(moments), B=-1) == E_SHAPE
    assert hip_lib.mtr_reconstruct_moments(p(g[0]), p(g[1]), p(g[2]), B, J, p(moments), p(ws), need - 1, stream) == E_WORKSPACE
    assert absolute(B=0) == 0 and solve(p(moments), B=0) == 0              # an empty batch: OK, nothing launched
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all()) and bool(torch.isnan(ws).all())
    assert absolute(ws_bytes=need) == 0                                      # exactly the stated size is accepted
    torch.cuda.synchronize()
    assert torch.equal(out, kernels.reconstruct_absolute(*g, m)) and guards_are_nan(buf)
    assert bool(torch.isnan(ws[need // 8:]).all())                          # ... and nothing is written behind it
