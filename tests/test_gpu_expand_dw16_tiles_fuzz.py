"""GPU: K27h (csrc/expand_dw16_tiles.hip) on shapes drawn from the whole domain it accepts, with the drawing helpers of
tests/conv_fuzz.py: 40 cases from random.Random(a fixed seed), every one inside the domain BY CONSTRUCTION -- either
stride, Cin from 8 .. 48 in steps of 8, Cmid from 8 .. 80 in steps of 8, the plane from the list enumerated from the rule
and cut at 64 rows and columns (stride 1: W % 4 == 0, H W % 8 == 0, no plane K11 runs on its block kernel; stride 2: H
even, W % 8 == 0), B 1 or 2, an activation pair, either dtype -- plus one 128x128 stride-2 case with 8 expanded
channels, the largest plane and 1024 staged positions.  Nothing is drawn and rejected and no case is skipped: the chain
K13h + K11 accepts every one of them too (asserted).  y must have the chain's bits, and nothing outside it is written."""
import random

import pytest
import torch

import conv_fuzz
from conv_fuzz import ACTS, BF16, F16, _balanced, _bordered, _gen

pytestmark = pytest.mark.gpu

N = 40
SIDE = 64


def _block_plane(H, W):
    """kernels.k11_takes_block_kernel, restated (this module draws its cases before the package is imported)."""
    if H % 4 or W % 4:
        return False
    bw, bh = W // 4, H // 4
    return not (bw & (bw - 1) or bh & (bh - 1)) and bw <= 16 and bw * bh <= 64


def _in_domain(H, W, stride):
    if stride == 1:
        return W % 4 == 0 and (H * W) % 8 == 0 and not _block_plane(H, W)
    return H % 2 == 0 and W % 8 == 0


# (H, W, stride) of the whole domain, H and W up to 128
DOMAIN = [(H, W, s) for s in (1, 2) for H in range(1, 129) for W in range(4, 129, 4) if _in_domain(H, W, s)]
PLANES = [p for p in DOMAIN if p[0] <= SIDE and p[1] <= SIDE]
LARGEST = dict(B=1, K=16, M=8, H=128, W=128, stride=2, act1='hardswish', act2='relu', dtype=F16)


def _cases():
    rng = random.Random(2727)
    s1, s2 = [p for p in PLANES if p[2] == 1], [p for p in PLANES if p[2] == 2]
    planes = rng.sample(s1, N // 2) + rng.sample(s2, N // 2)
    rng.shuffle(planes)
    acts1, acts2 = _balanced(rng, ACTS, N), _balanced(rng, ACTS, N)
    dtypes, batches = _balanced(rng, [F16, BF16], N), _balanced(rng, [1, 2], N)
    out = []
    for i in range(N):
        H, W, s = planes[i]
        out.append(dict(B=batches[i], K=8 * rng.randint(1, 6), M=8 * rng.randint(1, 10), H=H, W=W, stride=s,
                        act1=acts1[i], act2=acts2[i], dtype=dtypes[i]))
    return out + [LARGEST]


CASES = _cases()


def _id(c):
    return (f"s{c['stride']}-{c['B']}x{c['K']}-{c['M']}x{c['H']}x{c['W']}-{c['act1']}-{c['act2']}-"
            f"{str(c['dtype'])[6:]}")


def test_the_draw_covers_the_domain(hip_lib):
    from metrabs_amd import kernels
    assert len(CASES) == N + 1 and len({_id(c) for c in CASES}) == N + 1
    # the enumerated list is the host query's domain, plane by plane and stride by stride
    domain = set(DOMAIN)
    for s in (1, 2):
        for H in range(1, 133):
            for W in range(1, 133):
                assert (hip_lib.mtr_expand_dw16_tiles_lds_bytes(2, 16, 24, H, W, s) > 0) == ((H, W, s) in domain), \
                    (H, W, s)
    for H in range(1, 133, 3):
        for W in range(1, 133):
            assert _block_plane(H, W) == kernels.k11_takes_block_kernel(H, W)
    drawn = [(c['H'], c['W'], c['stride']) for c in CASES]
    assert set(drawn) <= domain and len(set(drawn)) == N + 1
    assert all(c['B'] <= 2 and c['M'] <= 80 and c['H'] <= SIDE and c['W'] <= SIDE for c in CASES[:N])
    assert sum(s == 1 for _, _, s in drawn) == N // 2
    assert any(H % 4 for H, _, s in drawn if s == 1) and any(H % 4 == 2 for H, _, s in drawn if s == 2)
    assert any(W % 8 for _, W, s in drawn if s == 1)                       # a span that starts four positions early
    assert any((W // s) % 8 == 0 for _, W, s in drawn) and any((W // s) % 8 for _, W, s in drawn)   # both segment widths
    assert any(H // s > 8 // s and (H // s) % (8 // s) for H, _, s in drawn)    # several bands, the last one partial
    assert {c['dtype'] for c in CASES} == {F16, BF16} and {c['B'] for c in CASES} == {1, 2}
    assert {c['act1'] for c in CASES} == set(ACTS) == {c['act2'] for c in CASES}
    assert any(c['M'] % 32 for c in CASES) and any(c['M'] > 32 for c in CASES)
    assert any(c['K'] % 16 for c in CASES) and any(c['K'] > 32 for c in CASES) and any(c['K'] <= 16 for c in CASES)


@pytest.mark.parametrize('c', CASES, ids=_id)
def test_k27h_fuzz_has_the_chains_bits(c, hip_lib):
    from metrabs_amd import kernels
    B, K, M, H, W, s, dt = c['B'], c['K'], c['M'], c['H'], c['W'], c['stride'], c['dtype']
    g = _gen('cuda', 1000 + K + M + H)
    x = _bordered(torch.randn(B, K, H, W, device='cuda', generator=g), 8.0).to(dt)
    w1 = (torch.randn(M, K, device='cuda', generator=g) / K ** 0.5).to(dt)
    b1 = 0.5 * torch.randn(M, device='cuda', generator=g)
    wd = torch.randn(M, 1, 3, 3, device='cuda', generator=g) * 0.4
    b2 = torch.randn(M, device='cuda', generator=g)
    # inside the domain of K27h AND of the chain: no case is skipped
    assert hip_lib.mtr_expand_dw16_tiles_lds_bytes(B, K, M, H, W, s) > 0
    assert kernels.expand_depthwise16_tiles_supported(x, w1, s)
    assert kernels.conv1x1_16_supported(x, w1) and (s == 2 or not kernels.k11_takes_block_kernel(H, W))
    mid = kernels.conv1x1_bias_act16(x, w1, b1, c['act1'])
    want = kernels.depthwise3x3_bias_act(mid, wd, b2, c['act2'], s, 1)
    big, out = conv_fuzz.guarded_out((B, M, H // s, W // s), dt, 'cuda')
    y = kernels.expand_depthwise16_tiles(x, w1, b1, c['act1'], wd, b2, c['act2'], s, out=out)
    assert y is out and conv_fuzz.bands_intact(big), 'a write outside out'
    assert torch.equal(y, want), (_id(c), int((y != want).sum()))
