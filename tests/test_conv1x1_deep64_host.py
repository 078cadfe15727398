"""CPU: K13's 'deep64' configuration as far as it needs no GPU: its code and name, the plans of
the flagship's 1x1 GEMM classes at batch 64, the refusals of the host-only plan entry and of the _opts entry, and that
CPU tensors take the library path."""
import ctypes

import torch

from metrabs_amd import _lib, backbones, kernels

# EfficientNetV2-S at 256 px: (M, K, HW) of the 1x1 convolutions of stages 4 - 6 and the head
MOVED = [(256, 64, 1024), (128, 256, 256), (512, 128, 256), (128, 512, 256), (160, 768, 256), (960, 160, 256),
         (160, 960, 256), (256, 960, 64), (1536, 256, 64), (256, 1536, 64), (1280, 256, 64)]
# ... the class that tied, and the FusedMBConv projects (pinned to 'stream' / 'tall')
KEPT = {(768, 128, 256): ('wide', 2, 192, 128), (48, 96, 4096): ('stream', 2, 64, 256),
        (48, 192, 4096): ('stream', 2, 64, 256), (64, 192, 1024): ('tall', 2, 64, 32), (64, 256, 1024): ('tall', 2, 64, 32)}


def test_code_and_name():
    assert kernels.CONV1X1_CONFIGS['deep64'] == 5
    assert sorted(kernels.CONV1X1_CONFIGS.values()) == [-1, 0, 1, 2, 3, 4, 5]
    assert _lib.SIGNATURES['mtr_conv1x1_plan'] and _lib.SIGNATURES['mtr_conv1x1_bias_act_pre']


def test_plans_of_the_flagship_classes_at_batch_64():
    for M, K, HW in MOVED:
        assert kernels.conv1x1_plan(M, K, HW, 64) == ('deep64', 2, 64, 64), (M, K, HW)
        assert kernels.conv1x1_plan(M, K, HW, 2) == ('deep64', 2, 64, 64)   # a function of the class, not of B
    for (M, K, HW), plan in KEPT.items():
        assert kernels.conv1x1_plan(M, K, HW, 64) == plan, (M, K, HW)
    # forced, it resolves to itself for every shape
    for M, K, HW, B in [(8, 8, 4, 1), (48, 192, 4096, 64), (200, 132, 4, 3), (1536, 256, 64, 64), (70000, 4, 4, 1)]:
        assert kernels.conv1x1_plan(M, K, HW, B, 'deep64') == ('deep64', 2, 64, 64)
    # MobileNetV3's classes (batch 320) keep what they ran: none shares (M, K, HW) with the list above
    for M, K, HW in [(80, 184, 256), (480, 80, 256), (112, 672, 256), (160, 960, 64), (960, 160, 64), (1280, 960, 64),
                     (24, 72, 4096), (40, 120, 1024), (80, 240, 256)]:
        assert kernels.conv1x1_plan(M, K, HW, 320)[0] in ('tall', 'square', 'wide')
    assert backbones.ConvBiasAct.k13_slower == frozenset()


def test_plan_and_opts_refusals():
    lib = _lib.load()
    plan = (ctypes.c_int * 4)()
    null = ctypes.c_void_p(0)
    assert lib.mtr_conv1x1_plan(256, 1536, 64, 64, 5, null) == -1                        # MTR_E_NULL
    assert lib.mtr_conv1x1_plan(256, 1536, 64, 64, 9, ctypes.addressof(plan)) == -4      # MTR_E_PARAM
    assert lib.mtr_conv1x1_plan(256, 1536, 64, 64, 6, ctypes.addressof(plan)) == -4
    assert lib.mtr_conv1x1_plan(256, 1536, 64, 64, 5, ctypes.addressof(plan)) == 0 and list(plan) == [5, 2, 64, 64]
    assert lib.mtr_conv1x1_plan(256, 1536, 64, 64, -1, ctypes.addressof(plan)) == 0 and list(plan) == [5, 2, 64, 64]
    # the entry from before the prologue keeps its range of configurations (refused before anything is read)
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    for config in (4, 5):
        assert lib.mtr_conv1x1_bias_act_opts(p, 0, p, p, null, null, 0, 1, 8, 8, 16, p, null, config) == -4
        assert lib.mtr_conv1x1_bias_act_opts(null, 0, p, p, null, null, 0, 1, 8, 8, 16, p, null, config) == -1


def test_cpu_tensors_take_the_library_path():
    torch.manual_seed(0)
    m = backbones.ConvBiasAct(torch.nn.Conv2d(1536, 256, 1, bias=False), torch.zeros(256), None)
    x = torch.randn(1, 1536, 8, 8)
    assert not m.k13_takes(x)
    with torch.no_grad():
        y = m(x)
    assert m.last_path == 'library' and y.shape == (1, 256, 8, 8)
    assert torch.allclose(y, torch.nn.functional.conv2d(x, m.conv.weight), atol=1e-5)
