"""GPU, SURVEY.md section 8 row a11: the affine-latent options of Metrabs (transform_coords /
predict_all_and_latents / regularize_to_manifold; metrabs_pytorch/models/metrabs.py:23-44,52-62, TF twin
metrabs_tf/models/metrabs.py:24-45,54-63,80-81, tfu3d.linear_combine_points tfu3d.py:48-49) against goldens
minted by the reference's own Metrabs (oracle/gen_golden.py:gen_latent) and against the oracle."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import cases, cpu_ref

pytestmark = pytest.mark.gpu


def build_model(c, fused_head, affine=None):
    from metrabs_amd.config import MetrabsConfig
    from metrabs_amd.joint_info import JointInfo
    from metrabs_amd.models.metrabs import Metrabs
    cfg = MetrabsConfig.from_any(c['cfg'].as_dict())
    ji = JointInfo([f'j{i}' for i in range(c['n_joints'])], [[0, 1]])
    affine = dict(w1=c['w1'].numpy(), w2=c['w2'].numpy()) if affine is None else affine
    model = Metrabs(torch.nn.Identity(), ji, cfg, in_channels=c['weight'].shape[1], fused_head=fused_head,
                    affine_weights=affine)
    assert model.heatmap_heads.n_points == c['n_raw'] == model.n_raw_points
    with torch.no_grad():
        model.heatmap_heads.conv_final.weight.copy_(c['weight'][:, :, None, None])
        model.heatmap_heads.conv_final.bias.copy_(c['bias'])
    return model.cuda().eval()


@pytest.mark.parametrize('fused_head', ['auto', True, False])
@pytest.mark.parametrize('name', list(cases.LATENT_CASES))
def test_latent_model_vs_reference_golden_and_oracle(name, fused_head, hip_lib):
    g = load_golden(f'latent_{name}')
    c = cases.latent_case(name)
    # (another LAPACK build may round a handful of consistent_head_case's float64 -> float32 features
    #  differently: the checksum then still agrees to ~1e-12, as in test_gpu_parity_gates.py)
    assert cases.sha256_of(c['features'], c['weight'], c['bias'], c['K'], c['w1'], c['w2']) == str(g['input_sha256']) \
        or abs(float(c['features'].double().sum()) - float(g['features_checksum'])) <= \
        1e-9 * max(1.0, abs(float(g['features_checksum']))), 'the seeded inputs are not the golden\'s'
    model = build_model(c, fused_head)
    with torch.inference_mode():
        ours = model((c['features'].cuda(), c['K'].cuda())).cpu()
        port = cpu_ref.crop_model_from_features(c['features'], c['weight'], c['bias'], c['K'], c['n_raw'],
                                                c['cfg'], c['w2'])
    ref, truth = torch.from_numpy(g['poses3d']), torch.from_numpy(g['poses3d_fp64'])
    assert ours.shape == ref.shape == (len(c['features']), c['n_joints'], 3)
    e_ref, e_port, e_truth = (float((ours.double() - x.double()).abs().max()) for x in (ref, port, truth))
    print(f'[parity] latent {name} head={fused_head}: max |ours - reference| {e_ref:.2e} mm, vs oracle {e_port:.2e}, '
          f'vs fp64 {e_truth:.2e} (reference vs fp64 MPJPE {float(g["reference_vs_fp64_mpjpe_mm"]):.2e})')
    # the north-star bound on the reference's own output and on the oracle; the stored reference is itself
    # up to 8.8e-4 mm MPJPE (2.5e-3 max) from an fp64 evaluation, so ours-vs-fp64 is gated tighter beside it
    floor = float(g['reference_vs_fp64_mpjpe_mm'])
    assert cpu_ref.mpjpe(ours, ref) <= max(1e-3, 1.5 * floor)
    assert cpu_ref.mpjpe(ours, truth) <= 5e-4 and e_truth <= 2e-3 and e_ref <= 5e-3
    # the oracle evaluated HERE, on the GPU box's host: its lstsq / oneDNN path moves with the host and the thread
    # count (round 6: 1.13e-3 mm from ours in one of three runs of the same commit, the stored reference 3.96e-4 in all
    # three) -- gated by what it can soundly be: its own distance to the fp64 evaluation plus ours
    port_floor = cpu_ref.mpjpe(port, truth)
    print(f'[parity] latent {name}: oracle on this host vs fp64 {port_floor:.2e} mm MPJPE')
    assert cpu_ref.mpjpe(ours, port) <= port_floor + 5e-4 and port_floor <= 3e-3


def test_latent_prefix_of_the_head_is_the_full_heads_slice(hip_lib):
    """predict_all_and_latents keeps coords[:, :n_latents] (models/metrabs.py:52-54); the head computes just
    those points from the selected weight rows -- the same bits as computing all and slicing, on both paths."""
    c = cases.latent_case('all_and_latents_b8')
    for fused in (True, False):
        model = build_model(c, fused)
        heads = model.heatmap_heads
        feat = c['features'].cuda()
        with torch.inference_mode():
            full2, full3 = heads(feat)
            part2, part3 = heads(feat, first_points=c['n_latents'])
        assert part2.shape == (len(feat), c['n_latents'], 2) and part3.shape == (len(feat), c['n_latents'], 3)
        if fused:
            assert torch.equal(part2, full2[:, :c['n_latents']]) and torch.equal(part3, full3[:, :c['n_latents']])
        else:  # (the library GEMM may block N = 261 and N = 108 differently)
            assert float((part3 - full3[:, :c['n_latents']]).abs().max()) <= 1e-3
        with pytest.raises(ValueError):
            heads(feat, first_points=c['n_raw'] + 1)


@pytest.mark.parametrize('shape', [(1, 12, 17), (64, 32, 122), (7, 40, 555), (0, 12, 17)])
def test_linear_combine_points_kernel(shape, hip_lib):
    """mtr_linear_combine_points = einsum 'bjc,jJ->bJc' (tfu3d.py:48-49), f64 sums."""
    from metrabs_amd import kernels
    B, j_in, j_out = shape
    g = cases.gen(77)
    pts = torch.randn(B, j_in, 3, generator=g) * 800 + torch.tensor([0.0, 0.0, 3500.0])
    _, w = cases.affine_weights_case(j_out, j_in, 78)
    out = kernels.linear_combine_points(pts.cuda(), w.cuda()).cpu()
    want64 = torch.einsum('bjc,jJ->bJc', pts.double(), w.double())
    assert out.shape == (B, j_out, 3)
    if B:
        # one rounding of an f64 sum: within half a unit in the last place of every output (+ the last bits
        # in which two f64 summation orders may differ)
        spacing = (torch.nextafter(out.abs(), torch.full_like(out, float('inf'))) - out.abs()).double()
        assert bool(((out.double() - want64).abs() <= 0.5001 * spacing).all())
        assert float((out - cpu_ref.linear_combine_points(pts, w)).abs().max()) <= 6e-3  # the f32 einsum's own noise
    eye = kernels.linear_combine_points(pts.cuda(), torch.eye(j_in).cuda()).cpu()
    assert torch.equal(eye, pts)


def test_linear_combine_points_at_the_latent_limit(hip_lib):
    """J_in = 4096 latent points fill the kernel's 48 KiB of LDS: runs, within 1 ulp of the float64 einsum; 4097 is
    refused (MTR_E_SHAPE) with no launch."""
    from metrabs_amd import kernels
    g = cases.gen(79)
    pts = torch.randn(2, 4096, 3, generator=g) * 800 + torch.tensor([0.0, 0.0, 3500.0])
    w = torch.randn(4096, 3, generator=g) / 64
    out = kernels.linear_combine_points(pts.cuda(), w.cuda()).cpu()
    want64 = torch.einsum('bjc,jJ->bJc', pts.double(), w.double())
    spacing = (torch.nextafter(out.abs(), torch.full_like(out, float('inf'))) - out.abs()).double()
    assert out.shape == (2, 3, 3) and bool(((out.double() - want64).abs() <= spacing).all())
    poisoned = torch.full((2, 3, 3), float('nan'), device='cuda')
    with pytest.raises(RuntimeError, match=r'code -2'):
        kernels.linear_combine_points(torch.zeros(2, 4097, 3, device='cuda'), torch.zeros(4097, 3, device='cuda'), out=poisoned)
    torch.cuda.synchronize()
    assert bool(torch.isnan(poisoned).all())


def test_estimator_over_a_latent_model_with_graphs(hip_lib):
    """The latent crop model behind Pose3dEstimator (eager, then captured): one more launch inside the body,
    same results either way, and equal to the oracle's estimate_poses_batched over the oracle's latent model."""
    from metrabs_amd.config import MetrabsConfig
    from metrabs_amd.joint_info import JointInfo
    from metrabs_amd.models.metrabs import Metrabs
    from metrabs_amd.multiperson.multiperson_model import Pose3dEstimator
    case = cases.e2e_case('aug5')
    n_lat, J = 9, 17
    w1, w2 = cases.affine_weights_case(J, n_lat, 4242)
    ocfg = cpu_ref.HeadConfig(**dict(case['cfg'].as_dict(), predict_all_and_latents=True))
    head_w, head_b = cases.tiny_head_weights(cases.E2E_C, n_lat + J, ocfg.depth, 4243)
    model = Metrabs(case['backbone'], JointInfo(cases.COCO17, cases.COCO17_EDGES), MetrabsConfig.from_any(ocfg.as_dict()),
                    in_channels=cases.E2E_C, affine_weights=dict(w1=w1, w2=w2))
    with torch.no_grad():
        model.heatmap_heads.conv_final.weight.copy_(head_w[:, :, None, None])
        model.heatmap_heads.conv_final.bias.copy_(head_b)
    est = Pose3dEstimator(model.cuda().eval(), {'': dict(indices=list(range(J)), names=cases.COCO17,
                                                         edges=cases.COCO17_EDGES)}, None)
    args = (case['images'], case['boxes'], case['K'], case['dist'], case['extr'], case['world_up'], 55, case['ibs'],
            case['aa'], case['num_aug'], case['average_aug'], '', False)
    with torch.inference_mode():
        est.graph_batches = False
        eager = torch.cat(est._estimate_poses_batched(*args)['poses3d']).cpu()
        est.graph_batches = True
        graphed = [torch.cat(est._estimate_poses_batched(*args)['poses3d']).cpu() for _ in range(2)]
        assert est.graphs.stats['replays'] >= 1, est.graphs.last_capture_error
        backbone_cpu = cases.e2e_case('aug5')['backbone']
        crop_model = lambda inp: cpu_ref.crop_model_from_features(backbone_cpu(inp[0]), head_w, head_b, inp[1],
                                                                  n_lat + J, ocfg, w2)
        ref = cpu_ref.estimate_poses_batched(crop_model, cases.mirror_mapping(cases.COCO17), J, case['res'], *args[:11])
    assert torch.equal(eager, graphed[0]) and torch.equal(eager, graphed[1])
    r3 = torch.cat(ref['poses3d'])
    print(f'[parity] latent e2e from images: MPJPE {cpu_ref.mpjpe(eager, r3):.2e} mm max {float((eager - r3).abs().max()):.2e}')
    assert eager.shape == r3.shape and cpu_ref.mpjpe(eager, r3) <= 1e-2
