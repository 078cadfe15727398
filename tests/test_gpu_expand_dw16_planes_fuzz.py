"""GPU: K26h (csrc/expand_dw16_planes.hip) on shapes drawn from the whole domain it accepts, with the drawing helpers
of tests/conv_fuzz.py: 40 cases from random.Random(a fixed seed), every one inside the domain BY CONSTRUCTION -- Cin
from 8 .. 256 in steps of 8, Cmid from 8 .. 400 in steps of 8, the plane from the list enumerated from the rule (W % 4
== 0, H W % 8 == 0, H and W at most 32, H W at most 576, no plane K11 runs on its block kernel; 12x12 and 24x24 three
times each), B from 1 .. 3, an activation pair, either dtype, the mean wanted or not -- so nothing is drawn and
rejected and no case is skipped: the chain K13h + K11 accepts every one of them too (asserted).  y and the mean must
have the chain's bits, and nothing outside them is written."""
import random

import pytest
import torch

import conv_fuzz
from conv_fuzz import ACTS, BF16, F16, _balanced, _bordered, _gen

pytestmark = pytest.mark.gpu

N = 40


def _block_plane(H, W):
    """kernels.k11_takes_block_kernel, restated (this module draws its cases before the package is imported)."""
    if H % 4 or W % 4:
        return False
    bw, bh = W // 4, H // 4
    return not (bw & (bw - 1) or bh & (bh - 1)) and bw <= 16 and bw * bh <= 64


PLANES = [(H, W) for H in range(1, 33) for W in range(4, 33, 4)
          if (H * W) % 8 == 0 and H * W <= 576 and not _block_plane(H, W)]
NETWORK_PLANES = [(12, 12), (24, 24)]


def _cases():
    rng = random.Random(2626)
    planes = NETWORK_PLANES * 3 + rng.sample([p for p in PLANES if p not in NETWORK_PLANES], N - 6)
    rng.shuffle(planes)
    acts1, acts2 = _balanced(rng, ACTS, N), _balanced(rng, ACTS, N)
    dtypes, means = _balanced(rng, [F16, BF16], N), _balanced(rng, [True, True, False], N)
    batches = _balanced(rng, [1, 2, 3], N)
    out = []
    for i in range(N):
        H, W = planes[i]
        out.append(dict(B=batches[i], K=8 * rng.randint(1, 32), M=8 * rng.randint(1, 50), H=H, W=W, act1=acts1[i],
                        act2=acts2[i], dtype=dtypes[i], want_mean=means[i]))
    return out


CASES = _cases()


def _id(c):
    return (f"{c['B']}x{c['K']}-{c['M']}x{c['H']}x{c['W']}-{c['act1']}-{c['act2']}-{str(c['dtype'])[6:]}"
            f"{'-mean' if c['want_mean'] else ''}")


def test_the_draw_covers_the_domain(hip_lib):
    from metrabs_amd import kernels
    assert len(CASES) == N and len({_id(c) for c in CASES}) == N
    # the enumerated list is the host query's domain, plane by plane
    for H in range(1, 41):
        for W in range(1, 41):
            assert (hip_lib.mtr_expand_dw16_planes_lds_bytes(2, 16, 24, H, W) > 0) == ((H, W) in PLANES), (H, W)
            assert _block_plane(H, W) == kernels.k11_takes_block_kernel(H, W)
    drawn = [(c['H'], c['W']) for c in CASES]
    assert set(drawn) <= set(PLANES) and len(set(drawn)) == N - 4
    assert all(drawn.count(p) >= 3 for p in NETWORK_PLANES)
    assert any(H % 4 for H, _ in drawn) and any(H != W for H, W in drawn)
    assert any(H * W <= 160 for H, W in drawn) and any(160 < H * W <= 320 for H, W in drawn) \
        and any(H * W > 320 for H, W in drawn)   # all three tile configurations
    assert {c['dtype'] for c in CASES} == {F16, BF16} and {c['B'] for c in CASES} == {1, 2, 3}
    assert {c['act1'] for c in CASES} == set(ACTS) == {c['act2'] for c in CASES}
    assert any(c['M'] % 64 for c in CASES) and any(c['K'] % 16 for c in CASES) and any(c['K'] > 128 for c in CASES)


@pytest.mark.parametrize('c', CASES, ids=_id)
def test_k26h_fuzz_has_the_chains_bits(c, hip_lib):
    from metrabs_amd import kernels
    B, K, M, H, W, dt = c['B'], c['K'], c['M'], c['H'], c['W'], c['dtype']
    g = _gen('cuda', 1000 + K + M + H)
    x = _bordered(torch.randn(B, K, H, W, device='cuda', generator=g), 8.0).to(dt)
    w1 = (torch.randn(M, K, device='cuda', generator=g) / K ** 0.5).to(dt)
    b1 = 0.5 * torch.randn(M, device='cuda', generator=g)
    wd = torch.randn(M, 1, 3, 3, device='cuda', generator=g) * 0.4
    b2 = torch.randn(M, device='cuda', generator=g)
    # inside the domain of K26h AND of the chain: no case is skipped
    assert hip_lib.mtr_expand_dw16_planes_lds_bytes(B, K, M, H, W) > 0
    assert kernels.expand_depthwise16_planes_supported(x, w1)
    assert kernels.conv1x1_16_supported(x, w1) and not kernels.k11_takes_block_kernel(H, W)
    mid = kernels.conv1x1_bias_act16(x, w1, b1, c['act1'])
    want, wmean = kernels.depthwise3x3_bias_act(mid, wd, b2, c['act2'], 1, 1, want_mean=True)
    big, out = conv_fuzz.guarded_out((B, M, H, W), dt, 'cuda')
    got = kernels.expand_depthwise16_planes(x, w1, b1, c['act1'], wd, b2, c['act2'], want_mean=c['want_mean'],
                                            out=out)
    y, mean = got if c['want_mean'] else (got, None)
    assert y is out and conv_fuzz.bands_intact(big), 'a write outside out'
    assert torch.equal(y, want), (_id(c), int((y != want).sum()))
    if mean is not None:
        assert torch.equal(mean, wmean), (_id(c), int((mean != wmean).sum()))
