"""GPU: K28h (csrc/expand_dw16_k5.hip) on shapes drawn from the whole domain it accepts, with the drawing helpers of
tests/conv_fuzz.py: 40 cases from random.Random(a fixed seed), every one inside the domain BY CONSTRUCTION -- half per
stride, the plane from the list enumerated from the restated rule (tests/test_expand_dw16_k5_host.lds_rule) and cut at 40
rows and columns, Cin from 8 .. 48 and Cmid from 8 .. 80 in steps of 8 plus a few odd Cmid, B 1 or 2, balanced activation
pairs and dtypes -- plus the largest plane the rule admits, with 8 expanded channels.  Nothing is drawn and rejected and
no case is skipped: the chain K13h + K15 accepts every one of them too (asserted).  y and the mean must have the chain's
bits, and nothing outside y is written."""
import random

import pytest
import torch

import conv_fuzz
from conv_fuzz import ACTS, BF16, F16, _balanced, _bordered, _gen
from test_expand_dw16_k5_host import lds_rule

pytestmark = pytest.mark.gpu

N = 40
SIDE = 40

# (H, W, stride) of the whole domain: the rule's answer at 32 channels (the slice every plane of the domain can take)
DOMAIN = [(H, W, s) for s in (1, 2) for H in range(1, 117) for W in range(1, 117) if lds_rule(8, H, W, s)]
PLANES = [p for p in DOMAIN if p[0] <= SIDE and p[1] <= SIDE]
_H, _W, _S = max(DOMAIN, key=lambda p: (p[0] * p[1], p))
LARGEST = dict(B=1, K=16, M=8, H=_H, W=_W, stride=_S, act1='hardswish', act2='relu', dtype=F16)


def _cases():
    rng = random.Random(2828)
    s1, s2 = [p for p in PLANES if p[2] == 1], [p for p in PLANES if p[2] == 2]
    planes = rng.sample(s1, N // 2) + rng.sample(s2, N // 2)
    rng.shuffle(planes)
    acts1, acts2 = _balanced(rng, ACTS, N), _balanced(rng, ACTS, N)
    dtypes, batches = _balanced(rng, [F16, BF16], N), _balanced(rng, [1, 2], N)
    out = []
    for i in range(N):
        H, W, s = planes[i]
        M = 8 * rng.randint(1, 10) if i % 8 else rng.choice([9, 33, 47, 65])   # a few odd Cmid
        out.append(dict(B=batches[i], K=8 * rng.randint(1, 6), M=M, H=H, W=W, stride=s, act1=acts1[i], act2=acts2[i],
                        dtype=dtypes[i]))
    return out + [LARGEST]


CASES = _cases()


def _id(c):
    return (f"s{c['stride']}-{c['B']}x{c['K']}-{c['M']}x{c['H']}x{c['W']}-{c['act1']}-{c['act2']}-"
            f"{str(c['dtype'])[6:]}")


def test_the_draw_covers_the_domain(hip_lib):
    assert len(CASES) == N + 1 and len({_id(c) for c in CASES}) == N + 1
    # the enumerated list is the host query's domain, plane by plane and stride by stride, for a narrow and a wide layer
    domain = set(DOMAIN)
    for Cmid in (8, 72):
        for s in (1, 2):
            for H in range(1, 121):
                for W in range(1, 121):
                    assert (hip_lib.mtr_expand_dw16_k5_lds_bytes(2, 16, Cmid, H, W, s) > 0) == ((H, W, s) in domain), \
                        (Cmid, H, W, s)
    drawn = [(c['H'], c['W'], c['stride']) for c in CASES]
    assert set(drawn) <= domain and len(set(drawn)) == N + 1
    assert all(c['B'] <= 2 and c['M'] <= 80 and c['H'] <= SIDE and c['W'] <= SIDE for c in CASES[:N])
    assert sum(s == 1 for _, _, s in drawn[:N]) == N // 2
    assert (_H * _W, _S) == (28 * 52, 1) and all(H * W <= _H * _W for H, W, _ in DOMAIN)
    units = lambda H, W, s: -(-((H - 1) // s + 1) // (4 // s)) * (((W - 1) // s + 1) // 4)
    assert any(units(*p) > 64 for p in drawn) and any(units(*p) <= 2 for p in drawn)
    assert any(H * W > 256 for H, W, _ in drawn[:N])                         # phase 1 in more than one pass
    assert any(((H - 1) // s + 1) % (4 // s) for H, _, s in drawn)            # a last unit row with dead rows
    assert any(H != W for H, W, _ in drawn)
    assert {c['dtype'] for c in CASES} == {F16, BF16} and {c['B'] for c in CASES} == {1, 2}
    assert {c['act1'] for c in CASES} == set(ACTS) == {c['act2'] for c in CASES}
    assert any(c['M'] % 8 for c in CASES) and any(c['M'] > 64 for c in CASES) and any(c['M'] <= 32 for c in CASES)
    assert any(c['K'] % 16 for c in CASES) and any(c['K'] > 32 for c in CASES) and any(c['K'] <= 16 for c in CASES)


@pytest.mark.parametrize('c', CASES, ids=_id)
def test_k28h_fuzz_has_the_chains_bits(c, hip_lib):
    from metrabs_amd import kernels
    B, K, M, H, W, s, dt = c['B'], c['K'], c['M'], c['H'], c['W'], c['stride'], c['dtype']
    g = _gen('cuda', 1000 + K + M + H)
    x = _bordered(torch.randn(B, K, H, W, device='cuda', generator=g), 8.0).to(dt)
    w1 = (torch.randn(M, K, device='cuda', generator=g) / K ** 0.5).to(dt)
    b1 = 0.5 * torch.randn(M, device='cuda', generator=g)
    wd = torch.randn(M, 1, 5, 5, device='cuda', generator=g) * 0.25
    b2 = torch.randn(M, device='cuda', generator=g)
    # inside the domain of K28h AND of the chain: no case is skipped
    assert hip_lib.mtr_expand_dw16_k5_lds_bytes(B, K, M, H, W, s) > 0
    assert kernels.expand_depthwise16_k5_supported(x, w1, s)
    assert kernels.conv1x1_16_supported(x, w1) and kernels.depthwise5x5_supported(H, W, 2)
    mid = kernels.conv1x1_bias_act16(x, w1, b1, c['act1'])
    want, want_mean = kernels.depthwise5x5_bias_act(mid, wd, b2, c['act2'], s, 2, want_mean=True)
    big, out = conv_fuzz.guarded_out(tuple(want.shape), dt, 'cuda')
    y, mean = kernels.expand_depthwise16_k5(x, w1, b1, c['act1'], wd, b2, c['act2'], s, want_mean=True, out=out)
    assert y is out and conv_fuzz.bands_intact(big), 'a write outside out'
    assert torch.equal(y, want), (_id(c), int((y != want).sum()))
    assert torch.equal(mean, want_mean), (_id(c), int((mean != want_mean).sum()))
