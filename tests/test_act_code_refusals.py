"""Every C entry point that takes an activation code answers MTR_E_PARAM for a code outside 0 .. 3, on the host and
before anything is enqueued: the kernels that take `act` at run time treat every unknown code as "none", so the entry
is the only place that can refuse one.  Host buffers and no GPU: a refusal precedes any launch, nothing is read."""
import ctypes

import pytest

from metrabs_amd import _lib

OK, E_PARAM = 0, -4
F32, F16 = 0, 1

_store = (ctypes.c_char * (1 << 16))()
_base = (ctypes.addressof(_store) + 255) & ~255
# 16-byte aligned and far enough apart that no tensor of the shapes below overlaps another
X, Y, W, W1, BIAS, BIAS1, OUT = (_base + i * 8192 for i in range(7))

# name -> call(act, B): the smallest shape the entry accepts (B 1, 8 channels, a 4 x 4 map; the stem 3 channels, 4 x 8)
ACT_ENTRIES = {
    'mtr_bias_act_nchw': lambda lib, act, B: lib.mtr_bias_act_nchw(Y, F32, BIAS, None, act, B, 8, 16, None),
    'mtr_bias_act_rowmean_nchw':
        lambda lib, act, B: lib.mtr_bias_act_rowmean_nchw(Y, F32, BIAS, act, B, 8, 16, OUT, None),
    'mtr_depthwise3x3_bias_act':
        lambda lib, act, B: lib.mtr_depthwise3x3_bias_act(X, F32, W, BIAS, act, B, 8, 4, 4, 1, 1, Y, None, None),
    'mtr_depthwise3x3_bias_act[stride 2]':
        lambda lib, act, B: lib.mtr_depthwise3x3_bias_act(X, F32, W, BIAS, act, B, 8, 8, 8, 2, 1, Y, None, None),
    'mtr_depthwise3x3_bias_act_padded':
        lambda lib, act, B: lib.mtr_depthwise3x3_bias_act_padded(X, F32, W, BIAS, act, B, 8, 4, 5, 1, 1, 0, 1, 1, Y,
                                                                 None, None),
    'mtr_depthwise3x3_blocks_bias_act':
        lambda lib, act, B: lib.mtr_depthwise3x3_blocks_bias_act(X, F32, W, BIAS, act, B, 8, 4, 4, Y, None, None),
    'mtr_depthwise5x5_bias_act_padded':
        lambda lib, act, B: lib.mtr_depthwise5x5_bias_act_padded(X, F32, W, BIAS, act, B, 8, 4, 4, 1, 2, 2, 2, 2, Y,
                                                                 None, None),
    'mtr_se_gate': lambda lib, act, B: lib.mtr_se_gate(X, W, BIAS, W1, BIAS1, act, 0, B, 8, 4, OUT, None),
    'mtr_se_gate_opts':
        lambda lib, act, B: lib.mtr_se_gate_opts(X, W, BIAS, W1, BIAS1, act, 0, B, 8, 4, OUT, None, 0, 0),
    'mtr_conv1x1_bias_act':
        lambda lib, act, B: lib.mtr_conv1x1_bias_act(X, F32, W, BIAS, None, None, act, B, 8, 8, 16, Y, None),
    'mtr_conv1x1_bias_act_opts':
        lambda lib, act, B: lib.mtr_conv1x1_bias_act_opts(X, F32, W, BIAS, None, None, act, B, 8, 8, 16, Y, None, 2),
    'mtr_conv1x1_bias_act_pre':
        lambda lib, act, B: lib.mtr_conv1x1_bias_act_pre(X, F32, W, BIAS, BIAS1, 2, None, None, act, B, 8, 8, 16, Y,
                                                         None, 4),
    'mtr_conv1x1_bias_act16':
        lambda lib, act, B: lib.mtr_conv1x1_bias_act16(X, F16, W, BIAS, None, None, act, B, 8, 8, 16, Y, None),
    'mtr_conv1x1_bias_act16_opts':
        lambda lib, act, B: lib.mtr_conv1x1_bias_act16_opts(X, F16, W, BIAS, None, None, act, B, 8, 8, 16, Y, None, 2),
    'mtr_conv1x1_bias_act_split':
        lambda lib, act, B: lib.mtr_conv1x1_bias_act_split(X, W, BIAS, BIAS1, 2, None, None, act, B, 8, 8, 16, Y,
                                                           None),
    'mtr_conv3x3_bias_act16':
        lambda lib, act, B: lib.mtr_conv3x3_bias_act16(X, F16, W, BIAS, None, act, B, 8, 8, 4, 8, 1, Y, None),
    'mtr_fused_mbconv16':
        lambda lib, act, B: lib.mtr_fused_mbconv16(X, F16, W, BIAS, act, W1, BIAS1, None, B, 8, 8, 8, 4, 8, 1, Y,
                                                   None),
    'mtr_stem_conv3x3s2':
        lambda lib, act, B: lib.mtr_stem_conv3x3s2(X, F32, 0, W, BIAS, F32, act, 0, B, 3, 8, 4, 8, Y, None),
    'mtr_conv3x3_winograd_bias_act':
        lambda lib, act, B: lib.mtr_conv3x3_winograd_bias_act(X, W, BIAS, None, act, B, 8, 8, 4, 4, Y, None),
}

# asserted for both codes where the entry's other refusals are (test_depthwise3x3_blocks_host.py)
PINNED_ELSEWHERE = {'mtr_depthwise3x3_blocks_bias_act_opts'}

# the two entries with an input activation: call(in_act, B), with an in_bias
IN_ACT_ENTRIES = {
    'mtr_conv1x1_bias_act_pre':
        lambda lib, in_act, B: lib.mtr_conv1x1_bias_act_pre(X, F32, W, BIAS, BIAS1, in_act, None, None, 2, B, 8, 8, 16,
                                                            Y, None, -1),
    'mtr_conv1x1_bias_act_split':
        lambda lib, in_act, B: lib.mtr_conv1x1_bias_act_split(X, W, BIAS, BIAS1, in_act, None, None, 2, B, 8, 8, 16, Y,
                                                              None),
}


def test_the_table_lists_every_entry_with_an_activation_code():
    import os
    import re
    header = open(os.path.join(os.path.dirname(_lib.__file__), '..', 'include', 'metrabs_hip.h')).read()
    declared = {m.group(1) for m in re.finditer(r'\bint\s+(mtr_\w+)\s*\(([^;]*?)\)\s*;', header, flags=re.S)
                if re.search(r'\bint act\b', m.group(2))}
    assert declared == {name.split('[')[0] for name in ACT_ENTRIES} | PINNED_ELSEWHERE
    with_in_act = {m.group(1) for m in re.finditer(r'\bint\s+(mtr_\w+)\s*\(([^;]*?)\)\s*;', header, flags=re.S)
                   if re.search(r'\bint in_act\b', m.group(2))}
    assert with_in_act == set(IN_ACT_ENTRIES)


@pytest.mark.parametrize('name', sorted(ACT_ENTRIES))
def test_unknown_act_is_refused(name):
    call, lib = ACT_ENTRIES[name], _lib.load()
    # the other arguments are acceptable: every entry makes its argument checks before "B == 0: nothing to do"
    assert [call(lib, act, 0) for act in range(4)] == [OK] * 4
    assert call(lib, -1, 1) == E_PARAM and call(lib, 4, 1) == E_PARAM


@pytest.mark.parametrize('name', sorted(IN_ACT_ENTRIES))
def test_unknown_in_act_is_refused(name):
    call, lib = IN_ACT_ENTRIES[name], _lib.load()
    assert [call(lib, in_act, 0) for in_act in range(4)] == [OK] * 4
    assert call(lib, -1, 1) == E_PARAM and call(lib, 4, 1) == E_PARAM
