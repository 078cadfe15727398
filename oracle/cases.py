"""TEST INFRASTRUCTURE: deterministic synthetic inputs for the oracle / golden vectors / parity tests.

Inputs follow SURVEY.md section 8(d): seeded torch.Generator (CPU RNG -- deterministic for a fixed
torch build; every golden file also stores a sha256 of its regenerated inputs so that an RNG change
is detected instead of silently comparing different data).
"""
import hashlib

import numpy as np
import torch
import torch.nn.functional as F

from oracle.cpu_ref import HeadConfig

COCO17 = ['nose', 'leye', 'reye', 'lear', 'rear', 'lsho', 'rsho', 'lelb', 'relb', 'lwri', 'rwri',
          'lhip', 'rhip', 'lkne', 'rkne', 'lank', 'rank']
COCO17_EDGES = [(0, 1), (0, 2), (1, 3), (2, 4), (5, 6), (5, 7), (7, 9), (6, 8), (8, 10), (5, 11),
                (6, 12), (11, 12), (11, 13), (13, 15), (12, 14), (14, 16)]


def mirror_mapping(names):
    """Left/right swap by leading 'l'/'r' (posepile JointInfo convention; see
    oracle/ref_harness.py:_JointInfoStub)."""
    index = {n: i for i, n in enumerate(names)}
    out = []
    for n in names:
        if n.startswith('l') and ('r' + n[1:]) in index:
            out.append(index['r' + n[1:]])
        elif n.startswith('r') and ('l' + n[1:]) in index:
            out.append(index['l' + n[1:]])
        else:
            out.append(index[n])
    return np.array(out, dtype=np.int64)


def sha256_of(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def gen(seed):
    return torch.Generator().manual_seed(int(seed))


# ------------------------------------------------------------------------------------ heads

HEAD_CASES = {
    # name: dict(B, J, D, H, W, sigma, dtype, cfg overrides)
    's256': dict(B=4, J=17, D=8, H=8, W=8, sigma=1.0, seed=101, cfg={}),
    's256_legacy': dict(B=4, J=17, D=8, H=8, W=8, sigma=3.0, seed=102,
                        cfg=dict(centered_stride=False, legacy_centered_stride_bug=True)),
    's256_peaked': dict(B=4, J=17, D=8, H=8, W=8, sigma=10.0, seed=103, cfg={}),
    'l384': dict(B=3, J=17, D=8, H=12, W=12, sigma=1.0, seed=104, cfg=dict(proc_side=384)),
    'l384_j122': dict(B=1, J=122, D=8, H=12, W=12, sigma=2.0, seed=105, cfg=dict(proc_side=384)),
    's256_d72': dict(B=2, J=17, D=72, H=8, W=8, sigma=1.0, seed=106, cfg=dict(depth=72)),
    's256_stride16': dict(B=2, J=17, D=8, H=16, W=16, sigma=2.0, seed=107,
                          cfg=dict(stride_test=16)),
    'odd160': dict(B=3, J=5, D=8, H=5, W=5, sigma=2.0, seed=108, cfg=dict(proc_side=160)),
    's256_fp16': dict(B=4, J=17, D=8, H=8, W=8, sigma=3.0, seed=109, dtype='float16', cfg={}),
    's256_j1': dict(B=2, J=1, D=8, H=8, W=8, sigma=1.0, seed=110, cfg={}),
    's256_spike': dict(B=2, J=17, D=8, H=8, W=8, sigma=1.0, seed=111, spike=60.0, cfg={}),
}


def head_case(name):
    c = dict(HEAD_CASES[name])
    cfg = HeadConfig(**c['cfg'])
    g = gen(c['seed'])
    n_out = c['J'] * (1 + c['D'])
    logits = torch.randn(c['B'], n_out, c['H'], c['W'], generator=g) * c['sigma']
    if c.get('spike'):
        # one dominant voxel per joint: exercises the exp range of the softmax
        for b in range(c['B']):
            for j in range(c['J']):
                d = int(torch.randint(0, c['D'], (1,), generator=g))
                h = int(torch.randint(0, c['H'], (1,), generator=g))
                w = int(torch.randint(0, c['W'], (1,), generator=g))
                logits[b, c['J'] + d * c['J'] + j, h, w] += c['spike']
                logits[b, j, h, w] += c['spike']
    if c.get('dtype') == 'float16':
        logits = logits.half()
    return logits, c['J'], cfg


HEADCONV_CASES = {
    's256_c64': dict(B=4, C=64, J=17, D=8, H=8, W=8, gain=1.0, seed=201, cfg={}),
    's256_c1280': dict(B=2, C=1280, J=17, D=8, H=8, W=8, gain=1.0, seed=202, cfg={}),
    's256_c1280_peaked': dict(B=2, C=1280, J=17, D=8, H=8, W=8, gain=20.0, seed=203, cfg={}),
    'l384_c1280': dict(B=2, C=1280, J=17, D=8, H=12, W=12, gain=4.0, seed=204,
                       cfg=dict(proc_side=384)),
    'r18_c512': dict(B=1, C=512, J=17, D=8, H=8, W=8, gain=4.0, seed=205, cfg={}),
    'l384_j122_c96': dict(B=2, C=96, J=122, D=8, H=12, W=12, gain=4.0, seed=206,
                          cfg=dict(proc_side=384)),
}


def default_conv_init(n_out, c_in, g):
    """torch.nn.Conv2d default init (kaiming_uniform a=sqrt(5) -> U(-1/sqrt(fan_in), ..))."""
    bound = 1.0 / np.sqrt(c_in)
    w = (torch.rand(n_out, c_in, generator=g) * 2 - 1) * bound
    b = (torch.rand(n_out, generator=g) * 2 - 1) * bound
    return w, b


def headconv_case(name):
    c = dict(HEADCONV_CASES[name])
    cfg = HeadConfig(**c['cfg'])
    g = gen(c['seed'])
    feat = torch.randn(c['B'], c['C'], c['H'], c['W'], generator=g)
    w, b = default_conv_init(c['J'] * (1 + c['D']), c['C'], g)
    return feat, w * c['gain'], b * c['gain'], c['J'], cfg


def consistent_head_case(B, C, J, hw, proc_side, D, amp, seed, spread=0.18):
    """Features + head parameters whose logits describe a PLAUSIBLE pose (a person filling most of
    the crop, 2.5 - 4.5 m from the camera), for the features -> poses3d parity gates.

    Why not random features x random weights: their heatmaps are nearly uniform, every joint decodes
    to the crop centre, the 2D and 3D spreads both vanish and the reference-point depth (their
    ratio, ptu3d.py:56-105) is ill-conditioned -- the median depth of such a batch is ~0 mm and even
    exactly rounded logits land 2e-3 mm from an fp64 evaluation.  No detector crop looks like that.

    Construction: conv_final keeps torch's default initialisation (W [N, C], bias); the target
    logits L* are Gaussian bumps of height `amp` (4: |logit| <= 5, 'low'; 25: 'peaked') around each
    joint's 2D / 3D heatmap position; the features of every position are the minimum-norm solution
    of W f = L* - bias plus a random N(0,1) vector projected onto W's null space, computed in
    float64 and rounded to float32 once.  So the features look like noise of unit scale (the
    K = C accumulation sees realistic magnitudes), the logits equal L* to rounding, and the poses
    are well conditioned.  -> (features [B,C,hw,hw] f32, weight [N,C], bias [N], K [B,3,3])"""
    g = gen(seed)
    w, b = default_conv_init(J * (1 + D), C, g)
    w, b = w.double(), b.double()
    f = (450 + 100 * torch.rand(B, generator=g)) * proc_side / 256
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = f, f, proc_side / 2, proc_side / 2, 1
    rel = (torch.randn(B, J, 3, generator=g, dtype=torch.float64) *
           torch.tensor([0.13, 0.17, 0.12], dtype=torch.float64)).clamp(-0.3, 0.3)
    u3 = 0.5 + rel                                   # (x, y, z) in heatmap units
    u2 = 0.5 + rel[..., :2] / (1.0 + 0.5 * rel[..., 2:])  # nearer joints project farther out
    gx = torch.linspace(0, 1, hw, dtype=torch.float64)
    gz = torch.linspace(0, 1, D, dtype=torch.float64)
    d2 = ((gx[None, None, None, :] - u2[..., 0, None, None]) ** 2 +
          (gx[None, None, :, None] - u2[..., 1, None, None]) ** 2)
    l2 = amp * torch.exp(-d2 / (2 * spread * spread))                                 # [B,J,h,w]
    d3 = ((gx[None, None, None, None, :] - u3[..., 0, None, None, None]) ** 2 +
          (gx[None, None, None, :, None] - u3[..., 1, None, None, None]) ** 2 +
          (gz[None, None, :, None, None] - u3[..., 2, None, None, None]) ** 2)
    l3 = amp * torch.exp(-d3 / (2 * spread * spread))                                 # [B,J,D,h,w]
    # conv_final's channel order: J 2D rows, then slice d of joint j at J + d*J + j
    target = torch.cat([l2, l3.permute(0, 2, 1, 3, 4).reshape(B, D * J, hw, hw)], dim=1)
    target = (target - b[None, :, None, None]).reshape(B, J * (1 + D), hw * hw)
    w_pinv = w.T @ torch.linalg.inv(w @ w.T)         # [C, N]
    noise = torch.randn(B, C, hw * hw, generator=g, dtype=torch.float64)
    feat = w_pinv @ target + noise - w_pinv @ (w @ noise)
    return feat.reshape(B, C, hw, hw).float(), w.float(), b.float(), K


def consistent_head_for_features(features, J, D, proc_side, amp, seed, spread=0.18, ridge=1e-6):
    """The converse of consistent_head_case for GIVEN features (a real backbone's output, [B,C,h,w] with
    B*h*w <= C): conv_final parameters under which THESE features describe a plausible pose -- the same
    Gaussian-bump target logits, W = T F^T (F F^T + ridge * mean diag)^-1 in float64 (a ridge keeps the
    weights small when the backbone's features are nearly dependent; the logits then equal the targets
    only approximately, which is all that is asked: peaked heatmaps, a person 2.5 - 4.5 m away), bias 0.
    -> (weight [N, C] f32, bias [N] f32, K [B,3,3])"""
    B, C, hw, hw2 = features.shape
    assert hw == hw2 and B * hw * hw <= C
    g = gen(seed)
    f = (450 + 100 * torch.rand(B, generator=g)) * proc_side / 256
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = f, f, proc_side / 2, proc_side / 2, 1
    rel = (torch.randn(B, J, 3, generator=g, dtype=torch.float64) *
           torch.tensor([0.13, 0.17, 0.12], dtype=torch.float64)).clamp(-0.3, 0.3)
    u3 = 0.5 + rel
    u2 = 0.5 + rel[..., :2] / (1.0 + 0.5 * rel[..., 2:])
    gx = torch.linspace(0, 1, hw, dtype=torch.float64)
    gz = torch.linspace(0, 1, D, dtype=torch.float64)
    d2 = ((gx[None, None, None, :] - u2[..., 0, None, None]) ** 2 +
          (gx[None, None, :, None] - u2[..., 1, None, None]) ** 2)
    l2 = amp * torch.exp(-d2 / (2 * spread * spread))
    d3 = ((gx[None, None, None, None, :] - u3[..., 0, None, None, None]) ** 2 +
          (gx[None, None, None, :, None] - u3[..., 1, None, None, None]) ** 2 +
          (gz[None, None, :, None, None] - u3[..., 2, None, None, None]) ** 2)
    l3 = amp * torch.exp(-d3 / (2 * spread * spread))
    target = torch.cat([l2, l3.permute(0, 2, 1, 3, 4).reshape(B, D * J, hw, hw)], dim=1)   # [B, N, h, w]
    T = target.permute(1, 0, 2, 3).reshape(J * (1 + D), B * hw * hw)                        # [N, B*HW]
    F = features.double().permute(1, 0, 2, 3).reshape(C, B * hw * hw)                        # [C, B*HW]
    gram = F.T @ F                                                                           # [BHW, BHW]
    gram = gram + ridge * gram.diagonal().mean() * torch.eye(gram.shape[0], dtype=torch.float64)
    w = torch.linalg.solve(gram, T.T).T @ F.T                                                # [N, C]
    return w.float(), torch.zeros(J * (1 + D)), K


# ---- the features -> poses3d parity gates (tests/test_gpu_parity_gates.py, bench.py's parity probe):
# every BASELINE.json config shape and the metric string's 72 depth bins.
# name: (B, C, J, map side, proc_side, depth bins, feature dtype)
PARITY_GATE_SHAPES = {
    'configs[0] ResNet-18 256 B=1': (1, 512, 17, 8, 256, 8, torch.float32),
    'configs[1] EffNetV2-S 256 B=64': (64, 1280, 17, 8, 256, 8, torch.float32),
    'configs[2] EffNetV2-L 384 B=32/GPU': (32, 1280, 17, 12, 384, 8, torch.float32),
    'configs[2] EffNetV2-L 384 B=256 on one GPU': (256, 1280, 17, 12, 384, 8, torch.float32),
    'configs[3] MobileNetV3 256, 8 boxes x 5 aug': (40, 1280, 17, 8, 256, 8, torch.float32),
    'configs[4] EffNetV2-L 384 f16 J=122 B=32/GPU': (32, 1280, 122, 12, 384, 8, torch.float16),
    'metric string: 72 depth bins, 256 px, B=64': (64, 1280, 17, 8, 256, 72, torch.float32),
}
PARITY_GATE_REGIMES = ('consistent_low', 'consistent_peaked', 'random_head')


def parity_gate_slug(name, regime):
    key = {'configs[0] ResNet-18 256 B=1': 'cfg0_r18_b1', 'configs[1] EffNetV2-S 256 B=64': 'cfg1_s_b64',
           'configs[2] EffNetV2-L 384 B=32/GPU': 'cfg2_l_b32', 'configs[2] EffNetV2-L 384 B=256 on one GPU': 'cfg2_l_b256',
           'configs[3] MobileNetV3 256, 8 boxes x 5 aug': 'cfg3_mnv3_b40',
           'configs[4] EffNetV2-L 384 f16 J=122 B=32/GPU': 'cfg4_l_f16_j122_b32',
           'metric string: 72 depth bins, 256 px, B=64': 'metric_d72_b64'}[name]
    return f'parity_{key}_{regime}'


def parity_gate_inputs(name, regime):
    """-> (features in the shape's dtype, weight [N,C] f32, bias, K [B,3,3]); seeded, CPU.
    consistent_low / consistent_peaked: consistent_head_case with bumps of 4 / 25; random_head: N(0,1)
    features x default-initialised conv_final x 8 (logits +-25) -- what a random-weight network emits."""
    B, C, J, hw, P, D, dtype = PARITY_GATE_SHAPES[name]
    seed = 9100 + sum(ord(c) for c in name)
    if regime == 'random_head':
        g = gen(seed)
        feat = torch.randn(B, C, hw, hw, generator=g)
        w, b = default_conv_init(J * (1 + D), C, g)
        w, b = w * 8.0, b * 8.0
        f = (450 + 100 * torch.rand(B, generator=g)) * P / 256
        K = torch.zeros(B, 3, 3)
        K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = f, f, P / 2, P / 2, 1
    else:
        amp = 4.0 if regime == 'consistent_low' else 25.0
        feat, w, b, K = consistent_head_case(B, C, J, hw, P, D, amp, seed)
    return feat.to(dtype), w, b, K


# ---- row a11: the affine-latent options of Metrabs (models/metrabs.py:23-44,52-62)
# name: (mode, B, C, n_joints, n_latents, map side, proc_side, depth bins, bump height, seed)
LATENT_CASES = {
    'transform_b8': ('transform_coords', 8, 256, 17, 12, 8, 256, 8, 4.0, 9501),
    'all_and_latents_b8': ('predict_all_and_latents', 8, 512, 17, 12, 8, 256, 8, 25.0, 9502),
    'all_and_latents_j60_384': ('predict_all_and_latents', 4, 1280, 60, 32, 12, 384, 8, 4.0, 9503),
    'regularize_b4': ('regularize_to_manifold', 4, 256, 17, 12, 8, 256, 8, 4.0, 9504),
}


def affine_weights_case(n_joints, n_latents, seed):
    """A synthetic affine-weights file: w1 [J, n_latents] (every latent point an affine combination of
    the joints: its column sums to 1) and w2 [n_latents, J] (every joint an affine combination of the
    latent points, negative weights included) -- what the reference's skeleton_conversion/*.npz hold."""
    g = gen(seed)
    w1 = torch.softmax(2.0 * torch.randn(n_joints, n_latents, generator=g), dim=0)
    r = 0.3 * torch.randn(n_latents, n_joints, generator=g)
    w2 = r - r.mean(dim=0, keepdim=True) + 1.0 / n_latents
    return w1.float().contiguous(), w2.float().contiguous()


def latent_case(name):
    """-> dict(cfg, features [B,C,h,w], weight [N,C], bias [N], K [B,3,3], w1, w2, n_joints, n_latents,
    n_raw): a plausible-pose head (consistent_head_case) over the model's RAW points."""
    mode, B, C, J, n_lat, hw, P, D, amp, seed = LATENT_CASES[name]
    cfg = HeadConfig(proc_side=P, depth=D, **{mode: True})
    n_raw = {'transform_coords': n_lat, 'predict_all_and_latents': n_lat + J,
             'regularize_to_manifold': J}[mode]
    feat, w, b, K = consistent_head_case(B, C, n_raw, hw, P, D, amp, seed)
    w1, w2 = affine_weights_case(J, n_lat, seed + 50)
    return dict(cfg=cfg, features=feat, weight=w, bias=b, K=K, w1=w1, w2=w2, n_joints=J, n_latents=n_lat,
                n_raw=n_raw)


# ------------------------------------------------------------------------------------ reconstruct

RECON_CASES = {
    'b64_j17': dict(B=64, J=17, seed=301, cfg={}),
    'b5_j122_384': dict(B=5, J=122, seed=302, cfg=dict(proc_side=384)),
    'b1_j17': dict(B=1, J=17, seed=303, cfg={}),
    'b8_legacy': dict(B=8, J=17, seed=304,
                      cfg=dict(centered_stride=False, legacy_centered_stride_bug=True)),
    'b8_weak': dict(B=8, J=17, seed=305, cfg=dict(weak_perspective=True)),
    'b6_nomix': dict(B=6, J=17, seed=306, cfg=dict(mix_3d_inside_fov=None)),
    'b4_outfov': dict(B=4, J=17, seed=307, cfg={}, all_out_of_fov=True),
}


def recon_case(name):
    """Synthetic *consistent* pose (SURVEY.md 8c KAT 5): pick ref point, K and rel pose, project,
    add prediction noise; ~10 % joints pushed out of the FOV."""
    c = dict(RECON_CASES[name])
    cfg_kw = dict(c['cfg'])
    mix = cfg_kw.pop('mix_3d_inside_fov', 0.5) if 'mix_3d_inside_fov' in cfg_kw else 0.5
    cfg = HeadConfig(**cfg_kw)
    cfg.mix_3d_inside_fov = mix
    g = gen(c['seed'])
    B, J, P = c['B'], c['J'], cfg.proc_side
    f = (450 + 100 * torch.rand(B, generator=g)) * (P / 256)
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0] = f
    K[:, 1, 1] = f * (0.98 + 0.04 * torch.rand(B, generator=g))
    K[:, 0, 2] = P / 2
    K[:, 1, 2] = P / 2
    K[:, 2, 2] = 1
    ref = torch.stack([
        200 * torch.randn(B, generator=g), 200 * torch.randn(B, generator=g),
        2000 + 3000 * torch.rand(B, generator=g)], dim=1)
    rel = torch.randn(B, J, 3, generator=g) * torch.tensor([350.0, 450.0, 250.0])
    abs3d = rel + ref[:, None]
    proj = abs3d[..., :2] / abs3d[..., 2:]
    coords2d = proj * torch.stack([K[:, 0, 0], K[:, 1, 1]], dim=1)[:, None] + K[:, None, :2, 2]
    coords2d = coords2d + 1.5 * torch.randn(B, J, 2, generator=g)
    rel = rel + 15 * torch.randn(B, J, 3, generator=g)
    push = torch.rand(B, J, generator=g) < 0.1
    coords2d = torch.where(push[..., None], coords2d * 0.02 - 3.0, coords2d)
    if c.get('all_out_of_fov'):
        coords2d[0] = -50.0 + torch.rand(J, 2, generator=g)
    return coords2d.contiguous(), rel.contiguous(), K, cfg


# ------------------------------------------------------------------------------------ images / warp

def weak_perspective_kat():
    """Hand-derived known answer for reconstruct_absolute(weak_perspective=True) (ptu3d.py:9-49,
    ptu.py:4-34) at the default config (FOV bounds [24, 232] px, mix 0.5), K = [[500,0,128],
    [0,500,128],[0,0,1]].

    Crop 0: four in-FOV joints on a rectangle + one joint outside the FOV (masked out of every
    mean).  Normalised 2D: x in {-0.04, 0.08}, y in {-0.12, 0.04} -> mean (0.02, -0.04), deviations
    (+-0.06, +-0.08): stdev2d = sqrt(4 (0.0036 + 0.0064) / 4) = 0.1.  Relative 3D: x in {-120, 180},
    y in {-220, 180} -> mean (30, -20), deviations (+-150, +-200): stdev3d = sqrt(4 (22500 + 40000) / 4)
    = 250; z mean 50.  Reference depth = 250 / 0.1 = 2500, ref = (0.02, -0.04, 1) 2500 - (30, -20, 50)
    = (20, -80, 2450).  In-FOV joints: 0.5 (rel + ref) + 0.5 (x_n, y_n, 1) (rel_z + 2450); the masked
    joint: rel + ref.
    Crop 1: no joint in the FOV -> masked means are nan_to_num(0 / 0) = 0, both stdevs
    max(sqrt(0 + 1e-10), 1e-5) -> depth 1, ref = (0, 0, 1); every joint: rel + (0, 0, 1).
    -> (coords2d [2,5,2], coords3d_rel [2,5,3], K [2,3,3], expected poses3d [2,5,3])"""
    K = torch.tensor([[500.0, 0, 128], [0, 500.0, 128], [0, 0, 1]]).repeat(2, 1, 1)
    c2d = torch.tensor([[[108.0, 68.0], [168.0, 68.0], [108.0, 148.0], [168.0, 148.0], [10.0, 128.0]],
                        [[5.0, 5.0], [250.0, 5.0], [5.0, 250.0], [250.0, 250.0], [128.0, 240.0]]])
    rel = torch.tensor([[[-120.0, -220.0, -100.0], [180.0, -220.0, 50.0], [-120.0, 180.0, 150.0],
                         [180.0, 180.0, 100.0], [999.0, -999.0, 999.0]],
                        [[10.0, 20.0, 30.0], [-40.0, 50.0, -60.0], [70.0, -80.0, 90.0],
                         [0.0, 0.0, 0.0], [-1.0, 2.0, -3.0]]])
    want = torch.tensor([[[-97.0, -291.0, 2350.0], [200.0, -300.0, 2500.0], [-102.0, 102.0, 2600.0],
                          [202.0, 101.0, 2550.0], [1019.0, -1079.0, 3449.0]],
                         [[10.0, 20.0, 31.0], [-40.0, 50.0, -59.0], [70.0, -80.0, 91.0],
                          [0.0, 0.0, 1.0], [-1.0, 2.0, -2.0]]])
    return c2d, rel, K, want


def box_consistency_kat():
    """Hand-derived known answers for is_pose_consistent_with_box (TF plausibility_check.py:66-84;
    PyTorch port :86-107): the pose's 2D bounding box is (10,10)-(50,90).
    -> (pose2d [6,3,2], boxes [6,5], expected bool [6])"""
    pose = torch.tensor([[10.0, 90.0], [50.0, 10.0], [30.0, 40.0]])
    rows = [
        ([0.0, 0.0, 60.0, 100.0, 1.0], True),     # intersection 40 x 80 = 3200 > 3000
        ([0.0, 0.0, 100.0, 100.0, 1.0], False),   # 3200 < 5000
        ([200.0, 0.0, 50.0, 50.0, 1.0], False),   # disjoint: relu -> 0
        ([10.0, 10.0, 80.0, 80.0, 0.3], False),   # 40 x 80 = 3200 > 3200 is false (strict >)
        ([30.0, 50.0, 40.0, 80.0, 0.9], False),   # x 30..50, y 50..90: 800 < 1600
        ([20.0, 20.0, 20.0, 60.0, 0.9], True),    # box inside the pose box: 1200 > 600
    ]
    boxes = torch.tensor([r[0] for r in rows])
    want = torch.tensor([r[1] for r in rows])
    return pose[None].repeat(len(rows), 1, 1), boxes, want


# ---- inputs of the recorded reference pins (tests/golden/oracle_pins.npz, oracle/gen_golden.py:gen_pins)
PIN_HEAD_BATCHES = [(7, 17, 8, 8, 256), (3, 29, 12, 8, 384), (2, 5, 4, 3, 128)]   # (B, J, H, D, proc_side)


def pin_head_batch(seed):
    """Random logits [B, J * (1 + D), H, H] and intrinsics of PIN_HEAD_BATCHES[seed] -> (logits, K, cfg)."""
    B, J, H, D, P = PIN_HEAD_BATCHES[seed]
    g = gen(900 + seed)
    cfg = HeadConfig(proc_side=P, depth=D)
    logits = torch.randn(B, J * (1 + D), H, H, generator=g) * 2
    K = torch.tensor([[500.0, 0, P / 2], [0, 510.0, P / 2], [0, 0, 1]]).repeat(B, 1, 1)
    return logits, K, cfg


def pin_box_consistency_inputs():
    """{'kat': box_consistency_kat's poses and boxes, 'random': 200 random poses and boxes}."""
    pose2d, boxes, _ = box_consistency_kat()
    g = gen(55)
    p = torch.rand(200, 17, 2, generator=g) * 300
    b = torch.cat([torch.rand(200, 2, generator=g) * 200, 50 + torch.rand(200, 2, generator=g) * 250,
                   torch.ones(200, 1)], dim=1)
    return {'kat': (pose2d, boxes), 'random': (p, b)}


def pin_geometry_inputs():
    """Points and distortion coefficients for distort / undistort_points, (forward, up) pairs for
    lookat_matrix (the second has forward parallel to up for its first row: the fallback branch)."""
    g = gen(77)
    pts = torch.randn(4, 5, 2, generator=g) * 0.4
    coeffs = [torch.zeros(4, 5), torch.tensor([DISTORTION_5] * 4), torch.tensor([DISTORTION_12] * 4)]
    fwd = torch.randn(6, 3, generator=g)
    fwd2 = fwd.clone()
    fwd2[0] = torch.tensor([0.0, 0.0, 2.0])
    lookat = [(fwd, torch.tensor([[0.0, -1.0, 0.0]]).repeat(6, 1)),
              (fwd2, torch.tensor([[0.0, 0.0, 1.0]]).repeat(6, 1))]
    return dict(points=pts, coeffs=coeffs, lookat=lookat)


def synth_images(n, h, w, seed):
    """uint8 [n,3,h,w]: even images are uniform noise (worst case for bilinear rounding), odd
    images are smooth gradients + mild noise."""
    g = gen(seed)
    imgs = torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, generator=g)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')
    for i in range(1, n, 2):
        base = torch.stack([
            127 + 100 * torch.sin(xx / 17.0 + i), 127 + 100 * torch.cos(yy / 23.0 - i),
            (xx + yy).float() % 256], dim=0)
        noise = torch.randint(-6, 7, (3, h, w), generator=g)
        imgs[i] = torch.clip(base + noise, 0, 255).to(torch.uint8)
    return imgs


def synth_boxes(n_images, h, w, max_boxes, seed, min_boxes=0):
    """list of [n_i,5] float32 boxes (x, y, w, h, conf=1); may contain empty entries."""
    g = gen(seed)
    out = []
    for _ in range(n_images):
        n = int(torch.randint(min_boxes, max_boxes + 1, (1,), generator=g))
        bw = (0.15 + 0.35 * torch.rand(n, generator=g)) * w
        bh = (0.3 + 0.6 * torch.rand(n, generator=g)) * h
        bx = torch.rand(n, generator=g) * (w - bw * 0.7) - 0.15 * bw
        by = torch.rand(n, generator=g) * (h - bh * 0.7) - 0.15 * bh
        out.append(torch.stack([bx, by, bw, bh, torch.ones(n)], dim=1).float())
    return out


DISTORTION_5 = (-0.1, 0.01, 1e-3, 1e-3, 0.0)
DISTORTION_12 = (-0.08, 0.012, 8e-4, -6e-4, 1e-3, 0.01, -2e-3, 1e-4, 3e-4, -2e-4, 1e-4, 2e-4)


def intrinsics_for(h, w, fov_degrees=55.0, jitter_seed=None):
    f = max(h, w) / (np.tan(np.deg2rad(fov_degrees) / 2) * 2)
    K = torch.tensor([[f, 0, w / 2], [0, f, h / 2], [0, 0, 1]], dtype=torch.float32)
    if jitter_seed is not None:
        g = gen(jitter_seed)
        K[0, 0] *= float(0.95 + 0.1 * torch.rand(1, generator=g))
        K[1, 1] *= float(0.95 + 0.1 * torch.rand(1, generator=g))
        K[0, 1] = float(0.5 * torch.randn(1, generator=g))  # a little skew
        K[0, 2] += float(3 * torch.randn(1, generator=g))
        K[1, 2] += float(3 * torch.randn(1, generator=g))
    return K


# ------------------------------------------------------------------------------------ e2e tiny model

class TinyBackbone(torch.nn.Module):
    """Deterministic stand-in for the CNN backbone (out of scope): /32
    average pool, 1x1 conv 3->C, tanh.  Cheap, and nearly order-independent in fp32 so that CPU
    and GPU features agree to ~1e-6."""

    def __init__(self, c_out, stride, seed):
        super().__init__()
        g = gen(seed)
        self.stride = stride
        self.proj = torch.nn.Conv2d(3, c_out, 1)
        with torch.no_grad():
            self.proj.weight.copy_(torch.randn(c_out, 3, 1, 1, generator=g) * 2.0)
            self.proj.bias.copy_(torch.randn(c_out, generator=g) * 0.5)

    def forward(self, image):
        x = F.avg_pool2d(image.float(), self.stride)
        return torch.tanh(self.proj(x * 2 - 1)) * 2.0


def tiny_head_weights(c_in, n_points, depth, seed, gain=6.0):
    g = gen(seed)
    w, b = default_conv_init(n_points * (1 + depth), c_in, g)
    return w * gain, b * gain


class PlausiblePoseBackbone(torch.nn.Module):
    """Stand-in backbone whose features, under the head of `plausible_pose_model`, describe a person
    filling most of the crop 1.5 - 4 m away -- for estimator tests that compare two EXECUTION ORDERS
    of the same crops (ranks, slices, graphs) and must not sit on the x / z singularity a random head
    produces (tests/test_gpu_sharded_estimator.py).

    The pose is a function of the CROP alone: twelve colour statistics of the crop (quadrant means per
    channel, float64, quantised to 2^-12 so that a reduction-order difference cannot move them) perturb
    a fixed base pose; the target logits are consistent_head_case's Gaussian bumps; the head is an
    matrix Q [N, C] of orthonormal rows (C = 160 >= N channels), so features = Q^T (target - bias),
    evaluated in float64 and rounded to float32 once: a crop's features do not depend on the batch it
    travels in."""

    def __init__(self, n_joints, depth, hw, seed, channels=160, amp=6.0, spread=0.18, zoom=1.5):
        super().__init__()
        g = gen(seed)
        n = n_joints * (1 + depth)
        assert channels >= n
        q, _ = torch.linalg.qr(torch.randn(channels, n, generator=g, dtype=torch.float64))
        self.n_joints, self.depth, self.hw, self.amp, self.spread, self.zoom = n_joints, depth, hw, amp, spread, zoom
        self.out_channels = channels
        self.register_buffer('q', q.T.contiguous())                                       # head weight [N, C]
        self.register_buffer('bias', (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1) * 0.05)
        base = (torch.randn(n_joints, 3, generator=g, dtype=torch.float64) *
                torch.tensor([0.13, 0.17, 0.12], dtype=torch.float64)).clamp(-0.25, 0.25)
        self.register_buffer('base', base)
        self.register_buffer('mix', torch.randn(12, n_joints * 3, generator=g, dtype=torch.float64))

    def head_parameters(self):
        return self.q.float(), self.bias.float()

    def forward(self, image):
        B, J, D, hw = image.shape[0], self.n_joints, self.depth, self.hw
        x = image.double()
        h2, w2 = x.shape[2] // 2, x.shape[3] // 2
        stats = torch.stack([x[:, :, :h2, :w2].mean((2, 3)), x[:, :, :h2, w2:].mean((2, 3)),
                             x[:, :, h2:, :w2].mean((2, 3)), x[:, :, h2:, w2:].mean((2, 3))], dim=2).reshape(B, 12)
        stats = torch.round(stats * 4096) / 4096
        rel = (self.base[None] + 0.06 * torch.tanh(3 * (stats - 0.3) @ self.mix).reshape(B, J, 3)).clamp(-0.3, 0.3)
        u3 = 0.5 + rel
        u2 = 0.5 + self.zoom * rel[..., :2] / (1.0 + 0.5 * rel[..., 2:])
        gx = torch.linspace(0, 1, hw, dtype=torch.float64, device=x.device)
        gz = torch.linspace(0, 1, D, dtype=torch.float64, device=x.device)
        s2 = 2 * self.spread * self.spread
        d2 = ((gx[None, None, None, :] - u2[..., 0, None, None]) ** 2 +
              (gx[None, None, :, None] - u2[..., 1, None, None]) ** 2)
        l2 = self.amp * torch.exp(-d2 / s2)
        d3 = ((gx[None, None, None, None, :] - u3[..., 0, None, None, None]) ** 2 +
              (gx[None, None, None, :, None] - u3[..., 1, None, None, None]) ** 2 +
              (gz[None, None, :, None, None] - u3[..., 2, None, None, None]) ** 2)
        l3 = self.amp * torch.exp(-d3 / s2)
        target = torch.cat([l2, l3.permute(0, 2, 1, 3, 4).reshape(B, D * J, hw, hw)], dim=1)
        target = target - self.bias[None, :, None, None]
        feat = torch.einsum('nc,bnp->bcp', self.q, target.reshape(B, -1, hw * hw))
        return feat.reshape(B, -1, hw, hw).float()


def with_plausible_pose_model(case, seed=977):
    """An e2e_case whose crop model is PlausiblePoseBackbone + its orthonormal-row head (C = 160 channels)."""
    cfg = case['cfg']
    bb = PlausiblePoseBackbone(17, cfg.depth, cfg.proc_side // cfg.stride_test, seed)
    w, b = bb.head_parameters()
    return dict(case, backbone=bb, head_w=w, head_b=b, C=bb.out_channels)


E2E_CASES = {
    # res 64 keeps the golden crops small; geometry/TTA/post-processing code paths are identical.
    'aug1': dict(seed=401, n_images=2, imh=120, imw=160, res=64, num_aug=1, aa=1, dist=None,
                 ibs=64, average_aug=True, extr=False, skeleton=False, jtm=False, known_k=False),
    'aug5': dict(seed=402, n_images=3, imh=120, imw=160, res=64, num_aug=5, aa=1, dist=None,
                 ibs=10, average_aug=True, extr=False, skeleton=False, jtm=False, known_k=True),
    'aug5_dist_aa2': dict(seed=403, n_images=2, imh=150, imw=200, res=64, num_aug=5, aa=2,
                          dist=DISTORTION_5, ibs=64, average_aug=False, extr=True, skeleton=True,
                          jtm=True, known_k=True),
    'aug4_dist12': dict(seed=404, n_images=2, imh=120, imw=160, res=64, num_aug=4, aa=1,
                        dist=DISTORTION_12, ibs=3, average_aug=True, extr=True, skeleton=False,
                        jtm=False, known_k=True),
    'aug2_aa8': dict(seed=409, n_images=3, imh=160, imw=200, res=32, num_aug=2, aa=8, dist=DISTORTION_5,
                     ibs=64, average_aug=True, extr=False, skeleton=False, jtm=False, known_k=True),
    'aug2_aa4_bigbox': dict(seed=405, n_images=1, imh=400, imw=600, res=32, num_aug=2, aa=4,
                            dist=None, ibs=64, average_aug=True, extr=False, skeleton=False,
                            jtm=False, known_k=False),
}

E2E_C = 24  # tiny backbone channels
# cases whose backbone outputs are stored too (golden e2efeat_*): the estimator's glue without the sampler
E2E_FEATURE_CASES = ('aug5', 'aug4_dist12', 'aug1', 'aug5_dist_aa2')
E2E_SKELETON = [0, 5, 6, 11, 12, 15, 16]


def e2e_case(name):
    c = dict(E2E_CASES[name])
    images = synth_images(c['n_images'], c['imh'], c['imw'], c['seed'])
    boxes = synth_boxes(c['n_images'], c['imh'], c['imw'], 3, c['seed'] + 1, min_boxes=1)
    if name == 'aug5':
        boxes[1] = boxes[1][:0]  # an image without detections (ragged edge case)
    if c['known_k']:
        K = torch.stack([intrinsics_for(c['imh'], c['imw'], 60.0, c['seed'] + 10 + i)
                         for i in range(c['n_images'])])
    else:
        K = torch.tensor([[[-1.0] * 3] * 3])
    dist = torch.tensor([list(c['dist'])], dtype=torch.float32) if c['dist'] else torch.zeros(1, 5)
    if c['extr']:
        g = gen(c['seed'] + 2)
        ang = 0.3 * torch.randn(3, generator=g)
        cx, sx, cy, sy = torch.cos(ang[0]), torch.sin(ang[0]), torch.cos(ang[1]), torch.sin(ang[1])
        rx = torch.tensor([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
        ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
        E = torch.eye(4)
        E[:3, :3] = rx @ ry
        E[:3, 3] = torch.tensor([100.0, -50.0, 800.0])
        extr = E[None]
        world_up = torch.tensor([0.0, 0.0, 1.0])
    else:
        extr = torch.eye(4)[None]
        world_up = torch.tensor([0.0, -1.0, 0.0])
    # stride res/8 -> an 8x8 heatmap, the EffNetV2-S/256 shape, at a tiny crop resolution
    cfg = HeadConfig(proc_side=c['res'], stride_train=c['res'] // 8, stride_test=c['res'] // 8)
    backbone = TinyBackbone(E2E_C, cfg.stride_test, c['seed'] + 3)
    w, b = tiny_head_weights(E2E_C, 17, cfg.depth, c['seed'] + 4)
    jtm = None
    if c['jtm']:
        g = gen(c['seed'] + 5)
        jtm = torch.eye(17) * 0.7 + 0.3 * torch.softmax(torch.randn(17, 17, generator=g), dim=0)
    skeleton = E2E_SKELETON if c['skeleton'] else list(range(17))
    return dict(images=images, boxes=boxes, K=K, dist=dist, extr=extr, world_up=world_up,
                cfg=cfg, backbone=backbone, head_w=w, head_b=b, jtm=jtm, skeleton=skeleton,
                num_aug=c['num_aug'], aa=c['aa'], ibs=c['ibs'], average_aug=c['average_aug'],
                res=c['res'])


WARP_CASES = {
    'nodist': dict(seed=501, dist=None, res=48),
    'dist5': dict(seed=502, dist=DISTORTION_5, res=48),
    'dist12': dict(seed=503, dist=DISTORTION_12, res=40),
}


def warp_case(name):
    """Direct inputs of warping.warp_images_with_pyramid: 2 images, 6 crops spanning all three
    pyramid levels and partially out-of-frame homographies."""
    c = dict(WARP_CASES[name])
    g = gen(c['seed'])
    imh, imw, res = 120, 160, c['res']
    images_u8 = synth_images(2, imh, imw, c['seed'])
    images = (images_u8.float() / 255) ** 2.2
    n = 6
    K = torch.stack([intrinsics_for(imh, imw, 55.0, c['seed'] + i) for i in range(n)])
    crop_scales = torch.tensor([1.6, 0.9, 0.45, 0.3, 0.2, 0.1])
    image_ids = torch.tensor([0, 1, 0, 1, 1, 0])
    hinvs = []
    for i in range(n):
        s = float(crop_scales[i])
        newK = torch.tensor([[K[i, 0, 0] * s, K[i, 0, 1] * s, res / 2],
                             [0, K[i, 1, 1] * s, res / 2], [0, 0, 1]])
        ang = 0.4 * torch.randn(3, generator=g)
        ca, sa = torch.cos(ang[2]), torch.sin(ang[2])
        rz = torch.tensor([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]])
        cb, sb = torch.cos(ang[0] * 0.3), torch.sin(ang[0] * 0.3)
        ry = torch.tensor([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
        hinvs.append(torch.linalg.inv(newK @ (rz @ ry)))
    hinv = torch.stack(hinvs)
    dist = (torch.tensor([list(c['dist'])] * n, dtype=torch.float32) if c['dist']
            else torch.zeros(n, 5))
    return dict(images_u8=images_u8, images=images, K=K, hinv=hinv, dist=dist,
                crop_scales=crop_scales, image_ids=image_ids, res=res)


# ------------------------------------------------------------------------- detector pre-processing

# name -> (n_images, h, w, seed): shrinking (antialiased) landscape / portrait / odd sizes, exact fit,
# enlarging (plain bilinear), and a size whose target is already a multiple of 32 (no padding)
DETPRE_CASES = {
    'qhd_270x480': (2, 270, 480, 21),
    'portrait_320x180': (1, 320, 180, 22),
    'odd_211x307': (2, 211, 307, 23),
    'exact_416x416': (1, 416, 416, 24),
    'small_100x64': (2, 100, 64, 25),
    'tiny_37x53': (1, 37, 53, 26),
    'nopad_512x832': (1, 512, 832, 27),
}


def detpre_case(name):
    n, h, w, seed = DETPRE_CASES[name]
    images = synth_images(n, h, w, seed)
    g = gen(seed + 1000)
    # detector answers in the padded network frame (x1, y1, x2, y2, conf); image 0 may be empty
    boxes = []
    for i in range(n):
        k = int(torch.randint(0 if i else 1, 5, (1,), generator=g))
        x1 = torch.rand(k, generator=g) * 300
        y1 = torch.rand(k, generator=g) * 300
        boxes.append(torch.stack([x1, y1, x1 + 20 + 100 * torch.rand(k, generator=g),
                                  y1 + 30 + 100 * torch.rand(k, generator=g),
                                  torch.rand(k, generator=g)], dim=1).float())
    return dict(images=images, net_boxes=boxes)


# ------------------------------------------------------------------ plausibility filter + pose NMS

# a standing person in camera space, mm (x right, y down, z forward): COCO-17 order
_TEMPLATE17 = [(0, -1650, 0), (30, -1680, -20), (-30, -1680, -20), (70, -1660, 40), (-70, -1660, 40),
               (180, -1400, 0), (-180, -1400, 0), (250, -1100, 20), (-250, -1100, 20),
               (270, -850, -30), (-270, -850, -30), (110, -900, 0), (-110, -900, 0),
               (120, -480, 10), (-120, -480, 10), (125, -60, 0), (-125, -60, 0)]

# name -> (n_images, max poses per image, num_aug, n_joints, seed)
FILTER_CASES = {
    'coco17_aug5': (3, 7, 5, 17, 41),
    'coco17_aug1': (2, 5, 1, 17, 42),
    'chain40_aug3': (2, 6, 3, 40, 43),
    'crowd_aug2': (1, 40, 2, 17, 44),
}


def filter_case(name):
    """Per image: distinct people, near-duplicates of some of them (same person detected twice:
    must be suppressed by the pose NMS), and poses that must fail each plausibility test (a bone
    5x too long, augmentation results that disagree, a pose far outside its detection box).
    Decisions are placed well away from the thresholds, so float summation order cannot flip them."""
    n_images, max_poses, A, J, seed = FILTER_CASES[name]
    g = gen(seed)
    if J == 17:
        template = torch.tensor(_TEMPLATE17, dtype=torch.float32)
        edges = list(COCO17_EDGES)
    else:  # a chain skeleton with J joints
        template = torch.cumsum(torch.randn(J, 3, generator=g) * torch.tensor([60.0, 90.0, 40.0]), dim=0)
        edges = [(i, i + 1) for i in range(J - 1)]
    tj = torch.tensor(edges)
    mean_bones = torch.norm(template[tj[:, 0]] - template[tj[:, 1]], dim=-1) * \
        (0.9 + 0.2 * torch.rand(len(edges), generator=g))
    f = 1000.0
    boxes, poses3d, poses2d, kinds = [], [], [], []
    for i in range(n_images):
        n_people = int(torch.randint(1, max(2, max_poses // 2) + 1, (1,), generator=g)) if i != 1 else 0
        items = []  # (pose [A,J,3], score, kind)
        for _ in range(n_people):
            base = template * (0.85 + 0.3 * torch.rand(1, generator=g)) + \
                torch.tensor([0.0, 900.0, 0.0]) + \
                (torch.rand(3, generator=g) - 0.5) * torch.tensor([3000.0, 300.0, 0.0]) + \
                torch.tensor([0.0, 0.0, 3000.0 + 3000.0 * float(torch.rand(1, generator=g))])
            pose = base[None] + torch.randn(A, J, 3, generator=g) * 8
            items.append((pose, 0.5 + 0.5 * float(torch.rand(1, generator=g)), 'person'))
            r = float(torch.rand(1, generator=g))
            if r < 0.4:  # the same person detected twice
                items.append((base[None] + torch.randn(A, J, 3, generator=g) * 12,
                              0.3 + 0.2 * float(torch.rand(1, generator=g)), 'duplicate'))
            elif r < 0.55:  # one bone far too long
                bad = pose.clone()
                bad[:, edges[3][0]] += torch.tensor([0.0, -2500.0, 0.0])
                items.append((bad + torch.tensor([900.0, 0.0, 400.0]), 0.6, 'long_bone'))
            elif r < 0.7 and A > 1:  # augmentation results disagree
                items.append((base[None] + torch.tensor([1500.0, 0.0, 800.0]) +
                              torch.randn(A, J, 3, generator=g) * 900, 0.55, 'inconsistent'))
            elif r < 0.85:  # plausible pose, but nowhere near its detection box
                items.append((pose + torch.tensor([-1200.0, 0.0, 300.0]), 0.7, 'off_box'))
        if i == 0 and items:  # every case holds at least one stretched skeleton
            bad = items[0][0].clone()
            bad[:, edges[3][0]] += torch.tensor([0.0, -2500.0, 0.0])
            items.insert(1, (bad + torch.tensor([900.0, 0.0, 400.0]), 0.6, 'long_bone'))
        items = items[:max_poses]
        order = torch.randperm(len(items), generator=g).tolist()
        items = [items[k] for k in order]
        if items:
            p3 = torch.stack([it[0] for it in items])
            p2 = f * p3[..., :2] / p3[..., 2:] + torch.tensor([960.0, 540.0])
            m2 = p2.mean(dim=1)
            lo, hi = m2.min(dim=1).values, m2.max(dim=1).values
            bx = torch.cat([lo - 20, hi - lo + 40, torch.tensor([[it[1]] for it in items])], dim=1)
            for k, it in enumerate(items):
                if it[2] == 'off_box':
                    bx[k, 0] += 3 * bx[k, 2]
        else:
            p3, p2, bx = torch.zeros(0, A, J, 3), torch.zeros(0, A, J, 2), torch.zeros(0, 5)
        boxes.append(bx.float())
        poses3d.append(p3.float())
        poses2d.append(p2.float())
        kinds.append([it[2] for it in items])
    return dict(boxes=boxes, poses3d=poses3d, poses2d=poses2d, edges=edges, mean_bones=mean_bones.float(),
                n_joints=J, kinds=kinds)


# ------------------------------------------------------------------ checkpoint format (row f.4)

def deterministic_state(state_dict, seed=0):
    """Fills a state_dict with values that depend only on each entry's NAME and shape (so two
    implementations with the same keys get the same weights regardless of construction order):
    conv weights ~ N(0, 1/fan_in), BN scale 0.8..1.2, BN var 0.5..1.5, everything else small."""
    import hashlib
    out = {}
    for k, v in state_dict.items():
        if v.dtype == torch.int64:  # num_batches_tracked
            out[k] = torch.zeros_like(v)
            continue
        h = int(hashlib.sha256(f'{seed}:{k}'.encode()).hexdigest()[:8], 16)
        g = torch.Generator().manual_seed(h)
        if k.endswith('running_var'):
            out[k] = 0.5 + torch.rand(v.shape, generator=g)
        elif k.endswith('running_mean'):
            out[k] = 0.1 * torch.randn(v.shape, generator=g)
        elif v.dim() == 4:
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]
            out[k] = torch.randn(v.shape, generator=g) * (1.0 / fan_in) ** 0.5
        elif k.endswith('.1.weight') or k.endswith('bn.weight'):
            out[k] = 0.8 + 0.4 * torch.rand(v.shape, generator=g)
        else:
            out[k] = 0.05 * torch.randn(v.shape, generator=g)
    return out


def backbone_probe_input():
    return torch.rand(2, 3, 96, 96, generator=gen(314))


def head_weights_as_consumed(w, feat_dtype):
    """The conv_final weights as the head's GEMM consumes them, for building the expected value on
    the CPU: with 16-bit features the weights are rounded to the feature dtype (what autocast does
    to conv_final in the reference's GPU path; the f16 / bf16 MFMA kernel and
    the library-GEMM path both do that)."""
    if feat_dtype == torch.float32:
        return w
    return w.to(feat_dtype).float()


# ------------------------------------------------------------------ post-head kernels (K5, K7, K8) on the paths
# the parity cases above do not reach: tests/test_posthead_cases_host.py checks the properties of these
# cases on the CPU, tests/test_gpu_reconstruct_paths.py, test_gpu_postprocess_boxes.py and test_gpu_filter.py
# run them through the kernels.

# (B, J): either side of the one-launch limit of mtr_reconstruct_absolute (B * J <= 16384)
RECON_PATH_SHAPES = {
    'b1030_j16': (1030, 16),    # 16 480: moments grid-stride (> 1024 crops), > 64 partial rows, B % 4 != 0
    'b65_j253': (65, 253),      # 16 445: J > 64 and J % 64 != 0
    'b128_j128': (128, 128),    # 16 384: the last shape of the one-launch kernel
    'b4097_j4': (4097, 4),      # 16 388: just over the limit with a tiny J
}
RECON_GENERAL_K_SHAPE = (300, 55)   # 16 500


def recon_paths_case(B, J, seed, general_k=False, mix_3d_inside_fov=0.5, centered_stride=True):
    """Synthetic consistent poses as tests/test_gpu_fuzz.py::test_reconstruct_fuzz builds them: a reference point
    2 - 4 m deep, a relative pose around it, its projection plus 2 px of noise; about three quarters of the joints
    land inside the FOV band.  general_k: skew, K[1,0] = 0.2 and a bottom row [g, h, 1] (inverse_rows01 of K5 is
    written for a general 3x3; every other case has [0, 0, 1]).
    -> (coords2d [B,J,2], coords3d_rel [B,J,3], K [B,3,3], cfg, ref [B,3])"""
    cfg = HeadConfig(centered_stride=centered_stride)
    cfg.mix_3d_inside_fov = mix_3d_inside_fov
    g = gen(seed)
    P = cfg.proc_side
    f = 450 + 100 * torch.rand(B, generator=g)
    K = torch.zeros(B, 3, 3)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2], K[:, 2, 2] = f, f * 1.01, P / 2, P / 2 + 1, 1
    K[:, 0, 1] = 0.3
    if general_k:
        K[:, 1, 0] = 0.2
        K[:, 2, 0] = RECON_GENERAL_K_BOTTOM[0] * (0.5 + torch.rand(B, generator=g))
        K[:, 2, 1] = RECON_GENERAL_K_BOTTOM[1] * (0.5 + torch.rand(B, generator=g))
    ref = torch.stack([150 * torch.randn(B, generator=g), 150 * torch.randn(B, generator=g),
                       2000 + 2000 * torch.rand(B, generator=g)], dim=1)
    rel = torch.randn(B, J, 3, generator=g) * torch.tensor([300.0, 400.0, 250.0])
    abs3d = rel + ref[:, None]
    c2d = (abs3d[..., :2] / abs3d[..., 2:]) * f[:, None, None] + P / 2 + 2 * torch.randn(B, J, 2, generator=g)
    return c2d.contiguous(), rel.contiguous(), K, cfg, ref


# (g, h) of the general-K case, each times a factor in 0.5 .. 1.5 per crop.  (1e-5 moves the fp64 answer by 2 bounds of
# tests/test_gpu_reconstruct_paths.py at the median joint; the case must move it by > 100: test_posthead_cases_host.py)
RECON_GENERAL_K_BOTTOM = (1e-3, -1e-3)


def f32_ulp_at(x):
    """Spacing of float32 at |x| (x float64): 2^(e - 24) for |x| = m 2^e, 0.5 <= m < 1."""
    _, e = torch.frexp(x.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), e - 24)


def recon_ulp_bound(out64, ref64):
    """The bound of tests/test_gpu_reconstruct_paths.py on |K5 - fp64| per joint, [B, J, 1]: 2 ulp of float32 at the
    joint's largest absolute coordinate + 0.5 ulp at the larger of that and the reference point's largest absolute
    coordinate -- 2.5 ulp at the joint wherever the reference point is no larger than the joint (derivation there)."""
    mj = out64.abs().amax(dim=-1, keepdim=True)
    mr = ref64.abs().amax(dim=-1)[:, None, None].expand_as(mj)
    return 2.0 * f32_ulp_at(mj) + 0.5 * f32_ulp_at(torch.maximum(mj, mr))


def recon_candidates_fp64(coords2d, coords3d_rel, intrinsics, cfg, mix_3d_inside_fov='cfg', weak_perspective=False):
    """The pieces of cpu_ref.reconstruct_absolute in float64: -> dict(ref [B,3], normalized [B,J,2],
    abs_3d_based = rel + ref, abs_2d_based = the back-projection (mixed when the mix is on), in_fov [B,J],
    out = what reconstruct_absolute returns)."""
    from oracle import cpu_ref
    if mix_3d_inside_fov == 'cfg':
        mix_3d_inside_fov = cfg.mix_3d_inside_fov
    c2d, rel = coords2d.double(), coords3d_rel.double()
    inv_k = torch.linalg.inv(intrinsics.double())
    normalized = (cpu_ref.to_homogeneous(c2d) @ inv_k.transpose(1, 2))[..., :2]
    in_fov = cpu_ref.is_within_fov(c2d, cfg)
    if weak_perspective:
        ref = cpu_ref.reconstruct_ref_weakpersp(normalized, rel, in_fov)
    else:
        ref = cpu_ref.reconstruct_ref_fullpersp(normalized, rel, in_fov)
    abs3 = rel + ref[:, None]
    abs2 = cpu_ref.back_project(normalized, rel[..., 2], ref[:, 2])
    if mix_3d_inside_fov is not None:
        abs2 = mix_3d_inside_fov * abs3 + (1 - mix_3d_inside_fov) * abs2
    return dict(ref=ref, normalized=normalized, abs_3d_based=abs3, abs_2d_based=abs2, in_fov=in_fov,
                out=torch.where(in_fov[..., None], abs2, abs3))


def recon_fov_edges_case(centered_stride):
    """A small consistent batch (no mixing) in which crop b's joints 0 .. 11 sit ON the FOV band's edges: x (joints
    0 - 5) or y (6 - 11) is exactly `lower`, the float32 next below it, the next above it, exactly `upper`, the next
    above and the next below; the other coordinate is mid-image.  is_within_fov is x >= lower && x <= upper.
    -> (coords2d, coords3d_rel, K, cfg, lower, upper, expect_inside [B,J] bool for the 12 edge joints (others: the
    oracle's own mask), edge_joints = 12)"""
    c2d, rel, K, cfg, _ = recon_paths_case(6, 17, 8800 + int(centered_stride), mix_3d_inside_fov=None,
                                           centered_stride=centered_stride)
    offset = 0.0 if centered_stride else -cfg.stride_train / 2
    lower = cfg.stride_train * 0.75 + offset
    upper = cfg.proc_side - cfg.stride_train * 0.75 + offset
    lo, up = torch.tensor(lower, dtype=torch.float32), torch.tensor(upper, dtype=torch.float32)
    inf = torch.tensor(float('inf'))
    values = [lo, torch.nextafter(lo, -inf), torch.nextafter(lo, inf), up, torch.nextafter(up, inf),
              torch.nextafter(up, -inf)]
    inside = [True, False, True, True, False, True]
    B = len(c2d)
    from oracle import cpu_ref
    expect = cpu_ref.is_within_fov(c2d, cfg).clone()
    for b in range(B):
        mid = 100.0 + 7.0 * b
        for k, v in enumerate(values):
            c2d[b, k] = torch.stack([v, torch.tensor(mid)])
            c2d[b, 6 + k] = torch.stack([torch.tensor(mid), v])
            expect[b, k] = expect[b, 6 + k] = inside[k]
    return c2d.contiguous(), rel, K, cfg, lower, upper, expect, 12


def pair_swap_mapping(J):
    """A mirror mapping that is not the identity for any joint count: 2i <-> 2i + 1 (a last odd joint maps to
    itself)."""
    m = torch.arange(J)
    even = torch.arange(0, J - 1, 2)
    m[even], m[even + 1] = even + 1, even
    return m


def per_box_cameras(n, seed):
    """K7 inputs that differ for every box of one call: extrinsics (rotation and translation), intrinsics and
    distortion -- box 0 none, box 1 DISTORTION_5, box 2 DISTORTION_12, cycling, each scaled per box so that no
    two boxes share a vector.  -> (K [n,3,3], distortion [n,12], extrinsics [n,4,4])"""
    g = gen(seed)
    K = torch.stack([intrinsics_for(1080, 1920, 55.0, seed + 31 * i) for i in range(n)])
    K[:, 0, 0] *= 0.8 + 0.4 * torch.rand(n, generator=g)
    K[:, 1, 1] *= 0.8 + 0.4 * torch.rand(n, generator=g)
    K[:, :2, 2] += 40 * torch.randn(n, 2, generator=g)
    d = torch.zeros(n, 12)
    for b in range(n):
        if b % 3 == 1:
            d[b, :5] = torch.tensor(DISTORTION_5) * (1 + 0.25 * b)
        elif b % 3 == 2:
            d[b] = torch.tensor(DISTORTION_12) * (1 + 0.25 * b)
    w = 0.3 * torch.randn(n, 3, generator=g)
    zero = torch.zeros(n)
    skew = torch.stack([torch.stack([zero, -w[:, 2], w[:, 1]], -1), torch.stack([w[:, 2], zero, -w[:, 0]], -1),
                        torch.stack([-w[:, 1], w[:, 0], zero], -1)], -2)
    E = torch.eye(4).repeat(n, 1, 1)
    E[:, :3, :3] = torch.linalg.matrix_exp(skew)
    E[:, :3, 3] = 500 * torch.randn(n, 3, generator=g)
    return K, d, E


def filter_grid_case(counts, A, J, seed, dup=(5, 4, 1), box_ok=(1, 0), scores=None, cols=32):
    """K8 inputs as tests/test_gpu_filter.py::test_filter_sizes_beyond_the_common_ones builds them, for several images
    and with the duplicates and the box test placed by rule: people on a grid 2.5 m x 3 m apart at 9 m (similarity 0
    between any two), 2 mm of noise per augmentation; pose i of an image is an exact duplicate (other noise) of pose
    i - dup[2] when i % dup[0] == dup[1]; a pose whose index is not box_ok[1] modulo box_ok[0] gets a detection box
    three box widths away (it fails is_pose_consistent_with_box and is invalid).  Scores: 0.9 - 0.0005 i (a
    duplicate scores below its original), or scores[image][i].  Decisions sit far from every threshold.
    -> dict(boxes, poses3d, poses2d: lists per image; edges, mean_bones, n_joints)"""
    g = gen(seed)
    edges = [(i, i + 1) for i in range(J - 1)]
    template = torch.cumsum(torch.randn(J, 3, generator=g) * torch.tensor([60.0, 90.0, 40.0]), dim=0)
    tj = torch.tensor(edges)
    mean_bones = torch.norm(template[tj[:, 0]] - template[tj[:, 1]], dim=-1)
    boxes, poses3d, poses2d = [], [], []
    for im, n in enumerate(counts):
        bases = []
        for i in range(n):
            base = template + torch.tensor([(i % cols) * 2500.0 - 1250.0 * cols, (i // cols) * 3000.0, 9000.0])
            if i % dup[0] == dup[1] and i >= dup[2]:
                base = bases[i - dup[2]].clone()
            bases.append(base)
        if n == 0:
            boxes.append(torch.zeros(0, 5)); poses3d.append(torch.zeros(0, A, J, 3)); poses2d.append(torch.zeros(0, A, J, 2))
            continue
        p3 = torch.stack(bases)[:, None].repeat(1, A, 1, 1) + torch.randn(n, A, J, 3, generator=g) * 2.0
        p2 = 1500.0 * p3[..., :2] / p3[..., 2:] + torch.tensor([960.0, 540.0])
        m2 = p2.mean(1)
        lo, hi = m2.min(1).values, m2.max(1).values
        sc = torch.tensor(scores[im], dtype=torch.float32) if scores is not None else 0.9 - 0.0005 * torch.arange(n)
        pad = 0.05 * (hi - lo)   # the pose's box covers 83 % of its detection: far above the 50 % of the box test
        bx = torch.cat([lo - pad, hi - lo + 2 * pad, sc[:, None]], dim=1)
        off = (torch.arange(n) % box_ok[0]) != box_ok[1]
        bx[off, 0] += 3 * bx[off, 2]
        boxes.append(bx.float()); poses3d.append(p3.float()); poses2d.append(p2.float())
    return dict(boxes=boxes, poses3d=poses3d, poses2d=poses2d, edges=edges, mean_bones=mean_bones, n_joints=J)


def filter_over256_case():
    """One image of 300 poses, J = 17, A = 2, every fifth a duplicate: 240 valid survivors of the NMS -- the
    256-thread strides of K8's rank and suppression passes take a second step (300 valid poses)."""
    return filter_grid_case([300], 2, 17, 9101)


def filter_cap_case():
    """One image of 200 poses, every fifth a duplicate: 160 distinct survivors, more than the cap of 150."""
    return filter_grid_case([200], 2, 17, 9102)


def filter_ties_case():
    """Equal scores on distinct poses and on exact duplicates (pose 4 duplicates 3, 9 duplicates 8): the lower index
    ranks first, as in the oracle's stable argsort."""
    scores = [[0.5, 0.7, 0.5, 0.6, 0.6, 0.5, 0.7, 0.7, 0.5, 0.5, 0.9, 0.5]]
    return filter_grid_case([12], 2, 17, 9103, scores=scores)


def filter_full_table_case():
    """Image 0 fills K8's per-image tables: 1024 poses, of which every eighth (i % 8 == 7, so index 1023 too) passes
    the box test -- 128 valid; pose i with i % 16 == 7 duplicates pose i - 8 (valid as well, higher score).  Image 1
    (24 poses by the same rules: 7, 15 and 23 valid, 23 a duplicate of 15) lies behind it, so its row_start and
    similarity offset follow a full table."""
    return filter_grid_case([1024, 24], 2, 17, 9104, dup=(16, 7, 8), box_ok=(8, 7))
