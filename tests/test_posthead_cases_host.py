"""CPU-only: the cases that tests/test_gpu_reconstruct_paths.py, test_gpu_postprocess_boxes.py and the K8 additions
of test_gpu_filter.py run through the kernels can tell a wrong kernel from a right one -- computed from the oracle
alone.  A case whose two candidate answers lie within the GPU test's bound of each other proves nothing there, so the
margins are asserted here (>= 100 times the bound), next to the properties the case builders promise, and next to an
emulation of K5's own arithmetic that keeps the GPU test's 2.5 ulp bound honest without a GPU."""
import numpy as np
import pytest
import torch

from oracle import cases, cpu_ref
from test_gpu_postprocess_boxes import BOX_CONFIGS, box_inputs, oracle_boxes

K7_BOUND_MM, K7_BOUND_PX = 1.5e-3, 2e-3   # the bounds of tests/test_gpu_postprocess.py


def recon_ulp_figures(out, c):
    """(max error in float32 ulp at the joint's largest coordinate over the joints whose reference point is no larger
    than the joint -- bound 2.5 --, the same over the other joints, their number, max error / bound over all)."""
    want = c['out']
    err = (out.double() - want).abs()
    ulp = cases.f32_ulp_at(want.abs().amax(dim=-1, keepdim=True))
    bound = cases.recon_ulp_bound(want, c['ref'])
    plain = (bound <= 2.5 * ulp).expand_as(err)
    z = torch.zeros(())
    return (float((err / ulp)[plain].max()), float(torch.cat([(err / ulp)[~plain], z[None]]).max()),
            int((~plain[..., 0]).sum()), float((err / bound).max()))


def emulate_k5(c2d, rel, K, cfg):
    """recon_solve_crop's output stage (metrabs_amd/csrc/reconstruct.hip) in float64 with its four float32 roundings:
    the reference point, rel + ref, the normalized coordinate, the final store.  The reference point itself comes
    from the float64 lstsq (the kernel's fp64 normal equations give the same minimiser)."""
    c = cases.recon_candidates_fp64(c2d, rel, K, cfg, mix_3d_inside_fov=None)
    rf = c['ref'].float().double()                              # (1)
    a3 = (rel.double() + rf[:, None]).float()                   # (2): ox, oy, oz; depth = (float)az
    depth = a3[..., 2:].double()
    nf = c['normalized'].float().double()                       # (3)
    back = torch.cat([nf * depth, depth], dim=-1)
    if cfg.mix_3d_inside_fov is not None:
        m = float(np.float32(cfg.mix_3d_inside_fov))
        back = m * a3.double() + (1.0 - m) * back
    return torch.where(c['in_fov'][..., None], back.float(), a3)  # (4)


RECON_CASES = [(name, B, J, False) for name, (B, J) in cases.RECON_PATH_SHAPES.items()] + \
    [('general_k',) + cases.RECON_GENERAL_K_SHAPE + (True,)]


@pytest.mark.parametrize('name,B,J,general_k', RECON_CASES, ids=[c[0] for c in RECON_CASES])
def test_recon_path_cases_have_the_promised_properties_and_k5s_arithmetic_meets_the_bound(name, B, J, general_k):
    c2d, rel, K, cfg, ref = cases.recon_paths_case(B, J, 8700 + J, general_k=general_k)
    assert (B * J > 16384) == (name != 'b128_j128')
    share = float(cpu_ref.is_within_fov(c2d, cfg).float().mean())
    assert 0.6 <= share <= 0.9, share
    assert float(ref[:, 2].min()) >= 2000 and float(ref[:, 2].max()) <= 4000
    c = cases.recon_candidates_fp64(c2d, rel, K, cfg)
    want = c['out']
    # (the pieces are the oracle's own function; two runs of the float64 lstsq may differ in a last bit: 1e-12 mm)
    assert float((want - cpu_ref.reconstruct_absolute(c2d.double(), rel.double(), K.double(), cfg)).abs().max()) <= 1e-9
    ulps, ulps_cancel, n_cancel, worst = recon_ulp_figures(emulate_k5(c2d, rel, K, cfg), c)
    print(f'[parity] K5 arithmetic emulated on the CPU, {name}: max {ulps:.2f} ulp vs fp64 (FOV share {share:.2f}); '
          f'{n_cancel} joints smaller than their reference point: {ulps_cancel:.2f} ulp, {worst:.2f} of the bound')
    assert ulps <= 2.5 and worst <= 1.0


def test_general_k_case_depends_on_the_bottom_row():
    """With the bottom row of K replaced by [0, 0, 1] the fp64 answer moves by more than 100 bounds: a kernel whose
    inverse assumed that row could not pass the general-K test."""
    B, J = cases.RECON_GENERAL_K_SHAPE
    c2d, rel, K, cfg, _ = cases.recon_paths_case(B, J, 8700 + J, general_k=True)
    assert float(K[:, 1, 0].abs().min()) > 0 and float(K[:, 2, :2].abs().min()) > 0
    c = cases.recon_candidates_fp64(c2d, rel, K, cfg)
    want = c['out']
    K0 = K.clone()
    K0[:, 2, :2] = 0
    other = cases.recon_candidates_fp64(c2d, rel, K0, cfg)['out']
    ratio = ((want - other).abs().amax(-1, keepdim=True) / cases.recon_ulp_bound(want, c['ref'])).flatten()
    print(f'general K: bottom row moves the fp64 answer by {float(ratio.max()):.0f} bounds at most, '
          f'{float(ratio.median()):.0f} at the median joint')
    assert float(ratio.median()) > 100


@pytest.mark.parametrize('centered_stride', [True, False])
def test_fov_edge_case_sits_on_the_edges_and_its_candidates_differ(centered_stride):
    c2d, rel, K, cfg, lower, upper, expect, n_edge = cases.recon_fov_edges_case(centered_stride)
    assert (lower, upper) == ((24.0, 232.0) if centered_stride else (8.0, 216.0))
    assert c2d.dtype == torch.float32
    c = cases.recon_candidates_fp64(c2d, rel, K, cfg)
    assert torch.equal(c['in_fov'], expect)       # the oracle's own >= / <= at every edge joint
    e = c2d[:, :n_edge]
    on = ((e == lower) | (e == upper)).any(-1)
    ulp_off = ((e - lower).abs() < 1e-4) | ((e - upper).abs() < 1e-4)
    assert int(on.sum()) == 4 * len(c2d) and bool(ulp_off.any(-1).all())
    assert bool(expect[:, :n_edge].any()) and bool((~expect[:, :n_edge]).any())
    gap = (c['abs_2d_based'] - c['abs_3d_based']).abs().amax(-1, keepdim=True)[:, :n_edge]
    ratio = gap / cases.recon_ulp_bound(c['out'], c['ref'])[:, :n_edge]
    print(f'FOV edges (centered_stride={centered_stride}): the two candidates differ by >= {float(ratio.min()):.0f} bounds')
    assert float(ratio.min()) > 100


@pytest.mark.parametrize('cfg', BOX_CONFIGS, ids=[c['id'] for c in BOX_CONFIGS])
def test_per_box_cameras_tell_the_boxes_apart(cfg):
    """Give every box box 0's extrinsics (distortion): the oracle's poses3d (poses2d) of EVERY other box with another
    camera moves by more than 100 times the GPU test's bound."""
    inp = box_inputs(cfg)
    n = cfg['n']
    d = inp['dist']
    assert [bool((d[b] != 0).any()) for b in range(n)] == [b % 3 != 0 for b in range(n)]
    assert bool((d[1::3, 5:] == 0).all()) and bool((d[2::3, 5:] != 0).any())
    grow = max(1.0, cfg['J'] / 122) if cfg['jt'] else 1.0
    for avg in (True, False):
        o3, o2 = oracle_boxes(inp, avg)
        e3, _ = oracle_boxes(dict(inp, E=inp['E'][:1].repeat(n, 1, 1)), avg)
        _, d2 = oracle_boxes(dict(inp, dist=d[:1].repeat(n, 1)), avg)
        for b in range(1, n):
            m3 = float((o3[b] - e3[b]).abs().max())
            assert m3 > 100 * K7_BOUND_MM * grow, (b, m3)
            if b % 3:
                m2 = float((o2[b] - d2[b]).abs().max())
                assert m2 > 100 * K7_BOUND_PX * grow, (b, m2)


def _valid_and_uncapped(c, image=0):
    keep, masks = cpu_ref.filter_poses(c['boxes'], c['poses3d'], c['poses2d'], c['edges'], c['mean_bones'], order='score')
    idx = torch.argwhere(masks[image])[:, 0]
    sim = cpu_ref.compute_pose_similarity(c['poses3d'][image].mean(1)[idx])
    full = idx[cpu_ref.non_max_suppression_overlaps(sim, c['boxes'][image][idx, 4], 0.4, max_output_size=10 ** 6,
                                                    order='score')]
    return masks, keep, full


def test_filter_cases_have_the_promised_counts():
    masks, keep, full = _valid_and_uncapped(cases.filter_cap_case())
    assert len(full) == 160 > 150 and len(keep[0]) == 150 and keep[0].tolist() == full[:150].tolist()
    masks, _, full = _valid_and_uncapped(cases.filter_over256_case())
    assert int(masks[0].sum()) == 300 > 256 and len(full) == 240
    c = cases.filter_full_table_case()
    masks, _, full = _valid_and_uncapped(c)
    assert [len(b) for b in c['boxes']] == [1024, 24]
    assert int(masks[0].sum()) == 128 and bool(masks[0][1023]) and 1023 in full.tolist() and len(full) == 65
    assert torch.argwhere(masks[1])[:, 0].tolist() == [7, 15, 23]


def test_filter_ties_case_is_decided_by_the_index():
    c = cases.filter_ties_case()
    s = c['boxes'][0][:, 4]
    assert float(s[3]) == float(s[4]) and float(s[8]) == float(s[9])       # duplicates with equal scores
    assert len(set(s.tolist())) < len(s) - 2                                # ... and ties among distinct poses
    keep_i, _ = cpu_ref.filter_poses(c['boxes'], c['poses3d'], c['poses2d'], c['edges'], c['mean_bones'], order='index')
    keep_s, _ = cpu_ref.filter_poses(c['boxes'], c['poses3d'], c['poses2d'], c['edges'], c['mean_bones'], order='score')
    assert keep_i[0].tolist() == [0, 1, 2, 3, 5, 6, 7, 8, 10, 11]
    assert keep_s[0].tolist() == [10, 1, 6, 7, 3, 0, 2, 5, 8, 11]
