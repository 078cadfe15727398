"""GPU: K21 (csrc/conv3x3_split.hip) on shapes drawn from the whole domain it accepts, with the drawing helpers of
tests/conv_fuzz.py: 24 cases from random.Random(a fixed seed), every one inside the domain BY CONSTRUCTION -- Cin from
8 .. 320 in steps of 8, Cout from conv_fuzz._cout_slots past the kernel's 128-channel block, the map from
conv_fuzz._map_kinds with W a multiple of 4 and any H, B from 1 .. 5, the activations and the skip balanced -- so
nothing is drawn and rejected and no case is skipped.  Every case passes the fp64 bound of tests/test_gpu_conv3x3_split.py
on every element, writes nothing outside y, and the entry's acceptance agrees with mtr_conv3x3_split_lds_bytes.

The odd-numbered half of the cases draws Cin from 8 .. 32 (Cp <= 32): there the bound is a few 1e-4 of S, and the wrong
answers of conv_fuzz._Conv3x3.wrong -- the last input channel dropped, two taps swapped, the last bias shifted, the skip
added in front of the activation -- must lie OUTSIDE it on at least one element; the last bias is set to 3.0 so that no
relu can hide its shift.  At Cin = 320 the worst-case bound is too wide to tell a shifted bias apart, which is why those
checks are made on the small-Cin half by construction."""

import pytest
import torch

import conv_fuzz
from conv_fuzz import ACT_CODES, F32, HOST, N_CASES, _cout_slots, _draw_map, _map_kinds, _opt

pytestmark = pytest.mark.gpu


class K21(conv_fuzz._Conv3x3):
    name, seed = 'k21', 2101
    past = [m for m in range(129, 301) if m % 128]   # past one workgroup's 128-channel block

    def module(self):
        import test_gpu_conv3x3_split
        return test_gpu_conv3x3_split

    def _generate(self, rng):
        couts, kinds = _cout_slots(rng, self.past), _map_kinds(rng)
        acts, ress = self._epilogues(rng)
        cases = []
        for i in range(N_CASES):
            H, W = _draw_map(rng, 'tiny' if kinds[i] in ('tiny', 'span') else kinds[i], wstep=4)
            B = 1 if kinds[i] == 'tiny' else rng.randint(2, 5) if kinds[i] == 'span' else rng.randint(1, 5)
            K = 8 * rng.randint(1, 4) if i % 2 else 8 * rng.randint(1, 40)
            cases.append(dict(B=B, K=K, M=couts[i], H=H, W=W, stride=1, act=acts[i], residual=ress[i], dtype=F32,
                              tell_wrong=bool(i % 2)))
        return cases

    def inputs(self, c, device, guard=False, seed=0):
        inp = super().inputs(c, device, guard=guard, seed=seed)
        inp['b'][-1] = 3.0
        return inp

    def _args(self, c, inp):
        return inp['x'], inp['w'], inp['b'], c['act'], inp['r']

    def accept(self, lib, c, B=0, p=None):
        p = p or HOST
        return [lib.mtr_conv3x3_bias_act_split(p.X, p.W, p.B, _opt(c['residual'], p.R), ACT_CODES[c['act']], B, c['K'],
                                               c['M'], c['H'], c['W'], p.Y, None),
                0 if lib.mtr_conv3x3_split_lds_bytes(c['B'], c['K'], c['M'], c['H'], c['W']) > 0 else -2]

    def run(self, kernels, c, inp, out=None):
        ws = kernels.pack_conv3x3_split_weight(inp['w'])
        assert kernels.conv3x3_split_supported(inp['x'], ws), c
        return kernels.conv3x3_bias_act_split(inp['x'], ws, inp['b'], c['act'], residual=inp['r'], out=out)


KERNEL = K21()
CASES = KERNEL.cases()


def _id(c):
    return (f"{c['B']}x{c['K']}-{c['M']}x{c['H']}x{c['W']}-{c['act']}{'-skip' if c['residual'] else ''}"
            f"{'-wrong' if c['tell_wrong'] else ''}")


def test_the_draw_covers_the_domain():
    assert len(CASES) == N_CASES == 24
    assert all(c['K'] % 8 == 0 and 8 <= c['K'] <= 320 and c['W'] % 4 == 0 and 1 <= c['B'] <= 5 for c in CASES)
    assert {c['act'] for c in CASES} == set(conv_fuzz.ACTS) and {c['residual'] for c in CASES} == {False, True}
    assert any(c['M'] > 128 for c in CASES) and any(c['M'] < 8 for c in CASES) and any(c['M'] % 8 for c in CASES)
    assert any(c['K'] % 16 for c in CASES) and any(c['K'] > 128 for c in CASES)
    assert any(c['H'] % 2 for c in CASES) and any(c['W'] > 16 for c in CASES) and any(c['W'] <= 16 for c in CASES)
    assert sum(c['tell_wrong'] for c in CASES) == 12 and all(c['K'] <= 32 for c in CASES if c['tell_wrong'])


@pytest.mark.parametrize('i', range(N_CASES), ids=[_id(c) for c in CASES])
def test_k21_fuzz(i, hip_lib):
    from metrabs_amd import kernels
    c = CASES[i]
    # the entry (B = 0: every check, no launch) and the query agree: inside the domain, nothing is skipped
    assert KERNEL.accept(hip_lib, c) == [0, 0], c
    inp = KERNEL.inputs(c, 'cuda', guard=True, seed=i)
    big, out = conv_fuzz.guarded_out(KERNEL.out_shape(c), F32, 'cuda')
    got = KERNEL.run(kernels, c, inp, out=out)
    torch.cuda.synchronize()
    assert got is out and conv_fuzz.bands_intact(big), 'a write outside out'
    assert not torch.isnan(got).any()          # the NaN bands around x and the skip did not reach y
    KERNEL.check(c, inp, got)
    if c['tell_wrong']:
        ref, bound = KERNEL.reference(c, inp)
        wrong = KERNEL.wrong(c, inp)
        assert {'last_channel', 'taps_swapped'} <= set(wrong)
        for kind, w in wrong.items():
            assert bool(((w - ref).abs() > bound).any()), (kind, c)
