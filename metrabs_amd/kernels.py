"""Tensor-level wrappers of the C-ABI (include/metrabs_hip.h): torch tensors in, torch tensors out,
kernels enqueued on torch's current HIP stream.  torch is used for device memory and streams only.
"""
import ctypes

import torch

from metrabs_amd import _lib
from metrabs_amd._lib import check, current_stream_ptr, dtype_code, require_cuda


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def softargmax_decode(logits, n_points, cfg, out=None, nhwc_staging=0):
    """logits [B, J*(1+D), H, W] (f32/f16/bf16, NCHW) -> (coords2d [B,J,2] px, coords3d_rel [B,J,3] mm).
    MetrabsHeads.forward after the conv (metrabs_pytorch/models/metrabs.py:78-85).
    nhwc_staging (channels_last logits; mtr_softargmax_decode_opts): 0 = the library's kernel choice, 1 = never the
    LDS-staged kernel, 2 = whenever the shape allows, 3 = as 2 with two crops per workgroup where that fills the waves; the same bits either way."""
    require_cuda(logits)
    lib = _lib.load()
    # torch channels_last logits (what a channels_last conv_final emits; the TF twin's
    # 'b h w (d j)' layout, metrabs_tf/models/metrabs.py:100-101) are decoded in place
    nhwc = _is_channels_last(logits)
    if not nhwc:
        logits = logits.contiguous()
    B, n_out, H, W = logits.shape
    J = int(n_points)
    D = n_out // J - 1
    if n_out != J * (1 + D) or D != cfg.depth:
        raise ValueError(f'logits have {n_out} channels, expected J*(1+depth) = {J * (1 + cfg.depth)}')
    if out is None:
        c2d = torch.empty(B, J, 2, device=logits.device, dtype=torch.float32)
        c3d = torch.empty(B, J, 3, device=logits.device, dtype=torch.float32)
    else:
        c2d, c3d = out
    hp = cfg.head_params()
    check(lib.mtr_softargmax_decode_opts(
        _ptr(logits), dtype_code(logits.dtype), _lib.MTR_NHWC if nhwc else _lib.MTR_NCHW, B, J, D, H, W,
        ctypes.byref(hp), int(nhwc_staging), _ptr(c2d), _ptr(c3d), current_stream_ptr(logits.device)),
        'mtr_softargmax_decode')
    return c2d, c3d


def reconstruct_workspace(B, J, device):
    n = _lib.load().mtr_reconstruct_workspace_bytes(int(B), int(J))
    return torch.empty((n + 7) // 8, device=device, dtype=torch.float64)


def reconstruct_absolute(coords2d, coords3d_rel, intrinsics, cfg, mix_3d_inside_fov='cfg',
                         weak_perspective=None, workspace=None, out=None):
    """ptu3d.reconstruct_absolute (metrabs_pytorch/ptu3d.py:9-33)."""
    require_cuda(coords2d, coords3d_rel, intrinsics)
    lib = _lib.load()
    coords2d = coords2d.contiguous().float()
    coords3d_rel = coords3d_rel.contiguous().float()
    intrinsics = intrinsics.contiguous().float()
    B, J = coords2d.shape[:2]
    if intrinsics.shape != (B, 3, 3) or coords3d_rel.shape != (B, J, 3):
        raise ValueError('shape mismatch between coords2d, coords3d_rel and intrinsics')
    if workspace is None:
        workspace = reconstruct_workspace(B, J, coords2d.device)
    if out is None:
        out = torch.empty(B, J, 3, device=coords2d.device, dtype=torch.float32)
    rp = cfg.recon_params(mix_3d_inside_fov, weak_perspective)
    check(lib.mtr_reconstruct_absolute(
        _ptr(coords2d), _ptr(coords3d_rel), _ptr(intrinsics), B, J, ctypes.byref(rp), _ptr(out),
        _ptr(workspace), workspace.numel() * 8, current_stream_ptr(coords2d.device)),
        'mtr_reconstruct_absolute')
    return out


def reconstruct_moments(coords2d, coords3d_rel, intrinsics, workspace=None):
    """-> f64 [3] = (sum normalized2d^2, sum rel_backproj^2, count) over this call's crops."""
    require_cuda(coords2d, coords3d_rel, intrinsics)
    lib = _lib.load()
    B, J = coords2d.shape[:2]
    if workspace is None:
        workspace = reconstruct_workspace(B, J, coords2d.device)
    moments = torch.zeros(3, device=coords2d.device, dtype=torch.float64)
    if B > 0:
        check(lib.mtr_reconstruct_moments(
            _ptr(coords2d), _ptr(coords3d_rel), _ptr(intrinsics), B, J, _ptr(moments),
            _ptr(workspace), workspace.numel() * 8, current_stream_ptr(coords2d.device)),
            'mtr_reconstruct_moments')
    return moments


def reconstruct_solve(coords2d, coords3d_rel, intrinsics, moments, cfg, mix_3d_inside_fov='cfg',
                      weak_perspective=None, out=None):
    require_cuda(coords2d, coords3d_rel, intrinsics, moments)
    lib = _lib.load()
    B, J = coords2d.shape[:2]
    if out is None:
        out = torch.empty(B, J, 3, device=coords2d.device, dtype=torch.float32)
    rp = cfg.recon_params(mix_3d_inside_fov, weak_perspective)
    check(lib.mtr_reconstruct_solve(
        _ptr(coords2d), _ptr(coords3d_rel), _ptr(intrinsics), B, J, ctypes.byref(rp),
        _ptr(moments), _ptr(out), current_stream_ptr(coords2d.device)), 'mtr_reconstruct_solve')
    return out


class Pyramid:
    """Linear-light image pyramid of the reference (multiperson_model.py:196 + warping.py:10-13).

    Two representations of level 0:
      * ``levels[0]`` f32 [N,3,H,W] (materialised -- what warping.warp_images_with_pyramid builds);
      * ``images_u8`` + ``lut``: level 0 stays the uint8 frame, decoded through the 256-entry gamma
        LUT inside the sampler (``levels[0]`` is None).  Same numbers, 64 % fewer pyramid bytes.
    ``levels[1]``, ``levels[2]`` are always f32 planes.  ``hwc``: ``images_u8`` is [N,3,H,W] over
    interleaved memory ([N,H,W,3]: torch channels_last, what decoders / numpy frames are) and is sampled
    as it lies -- the sampler then needs two gathers per sample instead of six."""

    def __init__(self, levels, images_u8=None, lut=None, hwc=False):
        self.levels = levels
        self.images_u8 = images_u8
        self.lut = lut
        self.hwc = bool(hwc)
        ref = images_u8 if levels[0] is None else levels[0]
        self.n, _, self.h, self.w = ref.shape
        self.device = ref.device


def frames_are_interleaved(images):
    """[N,3,H,W] frames whose memory is [N,H,W,3] (``x.permute(0, 3, 1, 2)`` of an HWC batch,
    ``memory_format=torch.channels_last``)?  Plain contiguous frames -- also the shapes where the two
    orders coincide -- are not."""
    return (images.ndim == 4 and images.shape[1] == 3 and not images.is_contiguous()
            and images.permute(0, 2, 3, 1).is_contiguous())


def _alloc_levels(n, h, w, device, with_level0=True):
    h1, w1 = h // 2, w // 2
    l0 = torch.empty(n, 3, h, w, device=device, dtype=torch.float32) if with_level0 else None
    l1 = torch.empty(n, 3, h1, w1, device=device, dtype=torch.float32)
    l2 = torch.empty(n, 3, h1 // 2, w1 // 2, device=device, dtype=torch.float32)
    return l0, l1, l2


# uint8 frames one sampler call can address (one 32-bit-offset buffer descriptor, csrc/warp.hip)
MAX_U8_FRAME_BYTES = (1 << 31) - 8


def build_pyramid(images_u8, materialize_level0=False, out=None):
    """uint8 [N,3,H,W] -> Pyramid: fused gamma decode (u8/255)**2.2 + two 2x2 box levels.  By
    default level 0 is NOT written as f32 (the sampler reads the uint8 frame through the LUT).
    Frames over interleaved memory (frames_are_interleaved) are used as they lie.
    out: a Pyramid made by this function over the SAME frame tensor: its levels and LUT are rewritten
    in place (fixed addresses for captured HIP graphs)."""
    require_cuda(images_u8)
    if images_u8.dtype != torch.uint8 or images_u8.ndim != 4 or images_u8.shape[1] != 3:
        raise ValueError('images must be uint8 [N,3,H,W]')
    hwc = frames_are_interleaved(images_u8) and not materialize_level0
    if not hwc:
        images_u8 = images_u8.contiguous()
    n, _, h, w = images_u8.shape
    lib = _lib.load()
    stream = current_stream_ptr(images_u8.device)
    build_u8 = lib.mtr_build_pyramid_u8_hwc if hwc else lib.mtr_build_pyramid_u8
    if materialize_level0:
        l0, l1, l2 = _alloc_levels(n, h, w, images_u8.device)
        check(lib.mtr_build_pyramid(_ptr(images_u8), n, h, w, _ptr(l0), _ptr(l1), _ptr(l2), stream),
              'mtr_build_pyramid')
        return Pyramid([l0, l1, l2])
    if out is not None:
        if out.images_u8 is None or out.images_u8.data_ptr() != images_u8.data_ptr() or \
                (out.n, out.h, out.w) != (n, h, w) or out.hwc != hwc:
            raise ValueError('build_pyramid(out=): the pyramid was not built over this frame tensor')
        check(build_u8(_ptr(images_u8), n, h, w, _ptr(out.lut), _ptr(out.levels[1]),
                       _ptr(out.levels[2]), stream), 'mtr_build_pyramid_u8')
        return out
    _, l1, l2 = _alloc_levels(n, h, w, images_u8.device, with_level0=False)
    lut = torch.empty(256, device=images_u8.device, dtype=torch.float32)
    check(build_u8(_ptr(images_u8), n, h, w, _ptr(lut), _ptr(l1), _ptr(l2), stream), 'mtr_build_pyramid_u8')
    return Pyramid([None, l1, l2], images_u8=images_u8, lut=lut, hwc=hwc)


def pyramid_from_level0(images_linear):
    """f32 linear-light [N,3,H,W] -> Pyramid (levels 1, 2 by 2x2 box filter)."""
    require_cuda(images_linear)
    l0 = images_linear.contiguous().float()
    n, _, h, w = l0.shape
    _, l1, l2 = _alloc_levels(n, h, w, l0.device, with_level0=False)
    check(_lib.load().mtr_pyramid_from_level0(_ptr(l0), n, h, w, _ptr(l1), _ptr(l2),
                                              current_stream_ptr(l0.device)),
          'mtr_pyramid_from_level0')
    return Pyramid([l0, l1, l2])


def pyramid_of_frames(images):
    """The pyramid of a call's frames [N,3,H,W] on the device.  uint8 frames: the fused LUT path (level 0 stays
    the frame).  Any other dtype -- the reference only ever says ``(images.float() / 255) ** 2.2``
    (multiperson_model.py:196), so float frames, also with non-integer values, are legal input -- by that very
    expression on the device and a materialised f32 level 0."""
    if images.dtype == torch.uint8:
        return build_pyramid(images)
    return pyramid_from_level0((images.float() / 255) ** 2.2)


def crop_geometry(boxes, intrinsics, distortion12, camspace_up, image_ids, aug_rotflipmat,
                  aug_scales, aug_gammas, res, antialias):
    """Per (aug, box): new intrinsics [A,n,3,3], R [A,n,3,3] and the warp parameter rows
    [A*n, 36] (multiperson_model.py:264-305,322-355)."""
    require_cuda(boxes, intrinsics, distortion12, camspace_up, image_ids)
    boxes = boxes.contiguous().float()
    n_box, n_aug = boxes.shape[0], aug_gammas.shape[0]
    dev = boxes.device
    new_k = torch.empty(n_aug, n_box, 3, 3, device=dev, dtype=torch.float32)
    rot = torch.empty(n_aug, n_box, 3, 3, device=dev, dtype=torch.float32)
    wp = torch.empty(n_aug * n_box, _lib.MTR_WARP_PARAM_FLOATS, device=dev, dtype=torch.float32)
    args = [intrinsics.contiguous().float(), distortion12.contiguous().float(),
            camspace_up.contiguous().float(), image_ids.contiguous().to(torch.int32),
            aug_rotflipmat.contiguous().float(), aug_scales.contiguous().float(),
            aug_gammas.contiguous().float()]
    if args[1].shape != (n_box, 12):
        raise ValueError('distortion coefficients must be zero-padded to [n_box, 12]')
    check(_lib.load().mtr_crop_geometry(
        _ptr(boxes), boxes.stride(0), *[_ptr(a) for a in args], n_box, n_aug, int(res),
        int(antialias), _ptr(new_k), _ptr(rot), _ptr(wp), current_stream_ptr(dev)),
        'mtr_crop_geometry')
    return new_k, rot, wp


# bytes of res*aa crops the antialias > 4 path holds at a time (_warp_crops_big_antialias)
MAX_BIG_CROP_BYTES = 1 << 30


def _check_warp_args(pyramid, warp_params, res, out_dtype, channels_last, out):
    """What warp_crops asks of its rows and of a caller's `out` (the kernels read 36 consecutive floats per crop and
    write a dense crop-major buffer: anything else would be sampled or written as garbage, silently)."""
    if not isinstance(warp_params, torch.Tensor) or not warp_params.is_cuda:
        raise ValueError('warp_crops: warp_params must be on the GPU')
    if warp_params.dtype != torch.float32 or warp_params.ndim != 2 or \
            warp_params.shape[1] != _lib.MTR_WARP_PARAM_FLOATS or not warp_params.is_contiguous():
        raise ValueError(f'warp_crops: warp_params must be float32 [n, {_lib.MTR_WARP_PARAM_FLOATS}], contiguous')
    if warp_params.device != pyramid.device:
        raise ValueError('warp_crops: warp_params and the pyramid are on different devices')
    if out is None:
        return
    n, res = warp_params.shape[0], int(res)
    ok = isinstance(out, torch.Tensor) and out.shape == (n, 3, res, res) and out.dtype == out_dtype and \
        out.device == warp_params.device
    # (the memory order asked for, crop-major and dense)
    if not ok or not (out.permute(0, 2, 3, 1) if channels_last else out).is_contiguous():
        layout = 'over [n, res, res, 3] memory (channels_last)' if channels_last else 'contiguous'
        raise ValueError(f'warp_crops: out must be {out_dtype} [n, 3, res, res] {layout} on the rows\' device')


def warp_crops(pyramid, warp_params, res, antialias=1, out_dtype=torch.float32,
               channels_last=False, out=None):
    """Pyramid + [n,36] warp rows -> crops [n,3,res,res] (NCHW) or NHWC memory when
    channels_last (returned as a logically-NCHW channels_last tensor).  warp_params: float32 [n,36] contiguous on
    the pyramid's device; out (optional): [n,3,res,res] of out_dtype in the layout asked for -- ValueError otherwise."""
    _check_warp_args(pyramid, warp_params, res, out_dtype, channels_last, out)
    n = warp_params.shape[0]
    dev = warp_params.device
    if antialias > 4:
        return _warp_crops_big_antialias(pyramid, warp_params, res, antialias, out_dtype, channels_last, out)
    if antialias not in (1, 2, 4):
        # (the reference warps at res*aa and only shrinks for 2, 4 and > 4: its reshape to
        #  [num_aug, n, 3, res, res] fails for 3, multiperson_model.py:307-316)
        raise ValueError(f'antialias_factor must be 1, 2, 4 or > 4 (got {antialias})')
    if out is None:
        if channels_last:
            out = torch.empty(n, res, res, 3, device=dev, dtype=out_dtype).permute(0, 3, 1, 2)
        else:
            out = torch.empty(n, 3, res, res, device=dev, dtype=out_dtype)
    l0, l1, l2 = pyramid.levels
    tail = (pyramid.n, pyramid.h, pyramid.w, _ptr(warp_params), n, int(res), int(antialias),
            dtype_code(out.dtype), _lib.MTR_NHWC if channels_last else _lib.MTR_NCHW, _ptr(out),
            current_stream_ptr(dev))
    if l0 is None:
        lib = _lib.load()
        warp_u8 = lib.mtr_warp_crops_u8_hwc if pyramid.hwc else lib.mtr_warp_crops_u8
        check(warp_u8(_ptr(pyramid.images_u8), _ptr(pyramid.lut), _ptr(l1), _ptr(l2), *tail),
              'mtr_warp_crops_u8')
    else:
        check(_lib.load().mtr_warp_crops(_ptr(l0), _ptr(l1), _ptr(l2), *tail), 'mtr_warp_crops')
    return out


def _warp_crops_big_antialias(pyramid, warp_params, res, antialias, out_dtype, channels_last, out):
    """antialias_factor > 4 (multiperson_model.py:312-315): sample at res*aa x res*aa in linear light
    (gamma exponent 1), shrink with aten's antialiased separable bilinear filter + the per-crop gamma
    (mtr_crops_shrink_antialiased).  The res*aa crops are 3 * (res*aa)^2 * 4 bytes each (50 MB at
    256 px, aa = 8): they are produced and consumed in chunks of <= MAX_BIG_CROP_BYTES (1 GiB)."""
    lib = _lib.load()
    n, dev = warp_params.shape[0], warp_params.device
    if 2 * antialias + 2 > 40:
        raise ValueError(f'antialias_factor {antialias} > 19 is not supported')
    big = int(res) * int(antialias)
    if out is None:
        out = (torch.empty(n, res, res, 3, device=dev, dtype=out_dtype).permute(0, 3, 1, 2) if channels_last
               else torch.empty(n, 3, res, res, device=dev, dtype=out_dtype))
    wp_lin = warp_params.clone()
    wp_lin[:, 33] = 1.0
    per = 3 * big * big * 4
    chunk = max(1, min(n, MAX_BIG_CROP_BYTES // per))
    flat_out = out.permute(0, 2, 3, 1) if channels_last else out  # the memory order, crop-major
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        tmp_big = warp_crops(pyramid, wp_lin[a:b].contiguous(), big, 1, torch.float32, False)
        ws = torch.empty(lib.mtr_crops_shrink_workspace_bytes(b - a, int(res), int(antialias)) // 4,
                         device=dev, dtype=torch.float32)
        check(lib.mtr_crops_shrink_antialiased(
            _ptr(tmp_big), _ptr(warp_params[a:b].contiguous()), b - a, int(res), int(antialias),
            dtype_code(out.dtype), _lib.MTR_NHWC if channels_last else _lib.MTR_NCHW,
            flat_out[a:b].data_ptr(), _ptr(ws), ws.numel() * 4, current_stream_ptr(dev)),
            'mtr_crops_shrink_antialiased')
    return out


def head_fused_supported(C, J, D, H, W, channels_last=False, dtype=torch.float32):
    """Shapes the fused projection+decode kernels cover; everything else goes through a library
    GEMM for the 1x1 conv followed by the HIP decode kernel (same results, logits via HBM).
    f32 features run the row-tile kernel: any map size, up to 80 depth bins.  f16 / bf16 features
    run the joint-group MFMA kernel (a joint's 1 + D rows inside a 64-row tile, maps of <= 256
    positions, C % 8 == 0) or, beyond those limits, the 16-bit row-tile kernel (C % 64 == 0, up to 80
    depth bins, any map size)."""
    if (H * W) % 4 != 0 or (channels_last and C % 4 != 0):
        return False
    if dtype == torch.float32:
        return D <= 80
    if H * W <= 256 and (1 + D) <= 64 and C % 8 == 0:
        return True
    return C % 64 == 0 and D <= 80


def head_auto_choice(C, J, D, H, W, channels_last=False, dtype=torch.float32):
    """MetrabsHeads(fused='auto'): True = the fused kernel, False = library 1x1 conv + mtr_softargmax_decode.
    A static table over (dtype, layout, C, H, W, J, D) read off the committed sweeps
    (profiles/*_fused_vs_library.txt, *_head_sweep.jsonl, r05c_f32_depth_sweep_fused_vs_library.jsonl) -- the
    batch size is deliberately NOT an input: a slice of a sharded batch, another rank and another process all
    take the path of the whole batch.  (INSIDE the fused path the library's launch plan may pick another kernel
    VARIANT by launch size -- f32 tile blocks, the 16-bit weights-in-registers kernel at >= 512 crops -- every one
    of which is bit-identical to the others on the same crop: tests/test_gpu_head.py asserts `torch.equal`
    across every dispatch choice, the default one at B = 512 against launches of 64 included.)
    The fused kernels are ahead on every shipped configuration (8x8 / 12x12 maps, 8 depth bins, 17 - 122
    joints, f32 / f16 / bf16); the library pair is kept for
      * 16-bit features on maps of more than 256 positions (the 16-bit row-tile kernel there is behind
        rocBLAS: 20x20 bf16 65 vs 39 us, 24x24 f16 37 vs 32 us),
      * f32 features on maps of >= 576 positions (24x24: 56 vs 50 us),
      * f32 features with more than 16 depth bins (round 5; the sweep at 17 joints, 8x8, B = 64 / 1024: 8 bins
        0.92 / 0.92 of the library pair's time, 16 bins 1.00 / 0.98, 24 bins 1.54 / 1.40, 32 bins 1.12 / 1.16,
        48 bins 1.14 / 1.15, 72 bins -- the metric string's shape -- 1.17 / 1.04, 80 bins 1.31 / 1.17: a
        joint's 1 + D rows no longer fit one 16-row tile and the multi-tile atoms quantise badly on 256 CUs).
        16-bit features keep the fused kernel there (72 bins, f16: 45 vs 70 us at 64 crops),
      * (round 6: the rule reads the LAYOUT) f32 channels_last features on maps of more than 64 positions: for them the
        library path is a plain GEMM (`F.linear` on the [B H W, C] matrix the features already are -- 2 - 5 x faster
        than the library's channels_last 1x1 convolution, which is what ran before) and is level with or ahead of the
        fused kernel from 12x12 maps on (64 / 256 crops of 12x12: 47 / 135 vs 52 / 158 us, 16x16 76 / 242 vs 69 / 250,
        20x20 104 / 401 vs 120 / 403; 8x8 with 8 / 16 bins stays fused: 23 / 64 vs 29 / 71, 34 / 121 vs 40 / 118;
        profiles/r06x_layout_rule*.jsonl)."""
    if not head_fused_supported(C, J, D, H, W, channels_last, dtype):
        return False
    hw = H * W
    if dtype == torch.float32:
        return (hw <= 64 if channels_last else hw < 576) and D <= 16
    return hw <= 256


def _is_channels_last(t):
    return (t.dim() == 4 and not t.is_contiguous()
            and t.is_contiguous(memory_format=torch.channels_last))


def head_pack_weights(weight2d, bias, n_points, depth, feat_dtype=torch.float32):
    """conv_final.weight [J*(1+D), C] + bias -> packed joint-major tiles for mtr_head_fused."""
    require_cuda(weight2d, bias)
    lib = _lib.load()
    weight2d = weight2d.contiguous().float()
    bias = bias.contiguous().float()
    n_out, C = weight2d.shape
    if n_out != n_points * (1 + depth):
        raise ValueError('weight rows != J*(1+depth)')
    nbytes = lib.mtr_head_packed_bytes(C, n_points, depth, dtype_code(feat_dtype))
    if nbytes == 0:
        raise ValueError(f'fused head does not support C={C}, J={n_points}, D={depth}')
    packed = torch.empty(nbytes // 4, device=weight2d.device, dtype=torch.float32)
    check(lib.mtr_head_pack_weights(_ptr(weight2d), _ptr(bias), C, n_points, depth,
                                    dtype_code(feat_dtype), _ptr(packed),
                                    current_stream_ptr(weight2d.device)), 'mtr_head_pack_weights')
    return packed


def head_fused(features, packed, C, n_points, cfg, out=None, rt_tiles=0, groups_per_workgroup=0,
               dma_staging=-1, rt_column_blocks=0, rt_k_groups=0, rt_loader=0, rt_split=0,
               workspace=None):
    """features [B,C,H,W] (f32/f16/bf16; NCHW-contiguous or torch channels_last = NHWC memory, which
    is consumed in place) -> (coords2d, coords3d_rel).  rt_tiles / groups_per_workgroup /
    dma_staging / rt_column_blocks / rt_k_groups / rt_loader / rt_split: explicit dispatch choices
    (mtr_head_options; defaults = the library's own).  workspace: None = a scratch tensor of
    mtr_head_workspace_bytes is allocated when the shape can use one (f32 maps of more than 64
    positions: column blocks over workgroups); False = none (mtr_head_fused_opts' behaviour); or a
    uint8 / float64 tensor to use."""
    require_cuda(features, packed)
    lib = _lib.load()
    nhwc = _is_channels_last(features)
    if not nhwc:
        features = features.contiguous()
    B, Cf, H, W = features.shape
    if Cf != C:
        raise ValueError(f'features have {Cf} channels, weights were packed for {C}')
    J, D = int(n_points), cfg.depth
    if out is None:
        c2d = torch.empty(B, J, 2, device=features.device, dtype=torch.float32)
        c3d = torch.empty(B, J, 3, device=features.device, dtype=torch.float32)
    else:
        c2d, c3d = out
    hp = cfg.head_params()
    layout = _lib.MTR_NHWC if nhwc else _lib.MTR_NCHW
    ws_ptr, ws_bytes = None, 0
    if workspace is not False:
        need = lib.mtr_head_workspace_bytes(dtype_code(features.dtype), layout, B, C, H, W, J, D)
        if need:
            if workspace is None:
                workspace = torch.empty((need + 7) // 8, device=features.device, dtype=torch.float64)
            require_cuda(workspace)
            ws_ptr, ws_bytes = _ptr(workspace), workspace.numel() * workspace.element_size()
    opts = _lib.head_options(rt_tiles, groups_per_workgroup, dma_staging, rt_column_blocks, rt_k_groups,
                             rt_loader, rt_split)
    check(lib.mtr_head_fused_ws(
        _ptr(features), dtype_code(features.dtype), layout, B, C, H, W, _ptr(packed), J, D,
        ctypes.byref(hp), ctypes.byref(opts), ws_ptr, ws_bytes, _ptr(c2d), _ptr(c3d),
        current_stream_ptr(features.device)), 'mtr_head_fused_ws')
    return c2d, c3d


def head_plan(B, C, H, W, n_points, depth, dtype=torch.float32, channels_last=False, have_workspace=True,
              **options):
    """Which kernel mtr_head_fused_ws takes for a launch (host-only; mtr_head_plan) -> dict(kernel=name,
    tiles_per_workgroup, column_blocks, split_column_blocks, workgroups, model_us) or None when the shape has
    no fused kernel.  options: as head_fused."""
    lib = _lib.load()
    opts = _lib.head_options(**{k: options[k] for k in ('rt_tiles', 'groups_per_workgroup', 'dma_staging',
                                                        'rt_column_blocks', 'rt_k_groups', 'rt_loader', 'rt_split')
                                if k in options})
    info = _lib.HeadPlanInfo()
    rc = lib.mtr_head_plan(dtype_code(dtype), _lib.MTR_NHWC if channels_last else _lib.MTR_NCHW, int(B), int(C),
                           int(H), int(W), int(n_points), int(depth), ctypes.byref(opts), int(bool(have_workspace)),
                           ctypes.byref(info))
    if rc != 0:
        return None
    return dict(kernel=_lib.HEAD_KERNEL_NAMES.get(info.kernel, str(info.kernel)),
                tiles_per_workgroup=info.tiles_per_workgroup, column_blocks=info.column_blocks,
                split_column_blocks=info.split_column_blocks, workgroups=int(info.workgroups),
                model_us=float(info.model_us))


def postprocess_poses(poses_crop, rot, should_flip, mirror_mapping, intrinsics, distortion12,
                      inv_extrinsics, joint_transform=None, skeleton=None, average_aug=True):
    """K7: crop-model output [A*n, J, 3] (or [A,n,J,3]) + R [A,n,3,3] -> (poses3d, poses2d) in the
    original camera / world frame: [n, S, 3|2] if average_aug else [n, A, S, 3|2]
    (multiperson_model.py:143-178,244-259)."""
    require_cuda(poses_crop, rot, intrinsics)
    dev = poses_crop.device
    A, n = rot.shape[0], rot.shape[1]
    poses_crop = poses_crop.contiguous().float().reshape(A, n, -1, 3)
    J = poses_crop.shape[2]
    # (.to is a no-op for tensors that already have the kernel's dtype on the device; callers on a
    # hot path pass cached uint8 / int32 device tensors)
    flip = should_flip.to(dev, torch.uint8).contiguous()
    mirror = mirror_mapping.to(dev, torch.int32).contiguous()
    jtm = joint_transform.to(dev, torch.float32).contiguous() if joint_transform is not None else None
    skel = skeleton.to(dev, torch.int32).contiguous() if skeleton is not None else None
    Jt = jtm.shape[1] if jtm is not None else J
    S = skel.numel() if skel is not None else Jt
    shape = (n, S) if average_aug else (n, A, S)
    p3 = torch.empty(*shape, 3, device=dev, dtype=torch.float32)
    p2 = torch.empty(*shape, 2, device=dev, dtype=torch.float32)
    check(_lib.load().mtr_postprocess_poses(
        _ptr(poses_crop), _ptr(rot.contiguous().float()), _ptr(flip), _ptr(mirror), _ptr(jtm), Jt,
        _ptr(skel), S, _ptr(intrinsics.contiguous().float()), _ptr(distortion12.contiguous().float()),
        _ptr(inv_extrinsics.contiguous().float()), A, n, J, int(bool(average_aug)), _ptr(p3),
        _ptr(p2), current_stream_ptr(dev)), 'mtr_postprocess_poses')
    return p3, p2


def linear_combine_points(points, weights, out=None):
    """points [B, J_in, 3], weights [J_in, J_out] -> [B, J_out, 3]: einsum 'bjc,jJ->bJc'
    (tfu3d.linear_combine_points, metrabs_tf/tfu3d.py:48-49; Metrabs.latent_points_to_joints,
    metrabs_tf/models/metrabs.py:80-81)."""
    require_cuda(points, weights)
    points = points.contiguous().float()
    weights = weights.contiguous().float()
    B, j_in = points.shape[:2]
    if points.shape[2] != 3 or weights.dim() != 2 or weights.shape[0] != j_in:
        raise ValueError(f'points {tuple(points.shape)} and weights {tuple(weights.shape)} do not match')
    j_out = weights.shape[1]
    if out is None:
        out = torch.empty(B, j_out, 3, device=points.device, dtype=torch.float32)
    if B == 0:
        return out
    check(_lib.load().mtr_linear_combine_points(_ptr(points), _ptr(weights), B, j_in, j_out, _ptr(out),
                                                current_stream_ptr(points.device)),
          'mtr_linear_combine_points')
    return out


# ------------------------------------------------------------------------------------------------
# K9: detector pre-processing (person_detector.py:14-54 minus the network)

def detector_geometry(h, w, input_size=416):
    """person_detector.py:15-20,26-29 -> _lib.DetectorGeom (host arithmetic, no GPU work)."""
    g = _lib.DetectorGeom()
    check(_lib.load().mtr_detector_geometry(int(h), int(w), int(input_size), ctypes.byref(g)),
          'mtr_detector_geometry')
    return g


DETECTOR_KERNELS = {'auto': 0, 'tile': 1, 'stream': 2}  # MTR_DETECTOR_KERNEL_*


def detector_preprocess(images_u8, geom=None, input_size=416, out=None, kernel='auto'):
    """images_u8 [N,3,H,W] uint8 (cuda) -> ([N,3,out_h,out_w] f32 as fed to the detector network,
    geometry).  person_detector.py:21-33.  `kernel`: 'auto' | 'tile' | 'stream' (identical bits; tests
    and timing name one)."""
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[1] != 3:
        raise ValueError('images must be uint8 [N,3,H,W]')
    require_cuda(images_u8)
    images_u8 = images_u8.contiguous()
    N, _, H, W = images_u8.shape
    g = geom if geom is not None else detector_geometry(H, W, input_size)
    if out is None:
        out = torch.empty(N, 3, g.out_h, g.out_w, device=images_u8.device, dtype=torch.float32)
    check(_lib.load().mtr_detector_preprocess_kernel(_ptr(images_u8), N, H, W, ctypes.byref(g),
                                                     DETECTOR_KERNELS[kernel], _ptr(out),
                                                     current_stream_ptr(images_u8.device)),
          'mtr_detector_preprocess_kernel')
    return out, g


def detector_scale_boxes(xyxy_conf, geom):
    """[n,5] (x1,y1,x2,y2,conf) in the padded network frame -> [n,5] (x,y,w,h,conf) in the image
    frame.  person_detector.py:47-54."""
    require_cuda(xyxy_conf)
    b = xyxy_conf.float().contiguous()
    out = torch.empty_like(b)
    check(_lib.load().mtr_detector_scale_boxes(_ptr(b), b.shape[0], ctypes.byref(geom), _ptr(out),
                                               current_stream_ptr(b.device)),
          'mtr_detector_scale_boxes')
    return out


# ------------------------------------------------------------------------------------------------
# K8: plausibility filter + pose NMS (plausibility_check.py / TF _filter_poses)

def filter_poses(poses3d, poses2d, boxes, n_per_image, edges, mean_bones, n_joints=None,
                 unbiased=False, order='index', max_output=150):
    """poses3d [P,A,J,3] (camera space, all model joints), poses2d [P,A,J,2], boxes [P,5], poses of
    image i contiguous with n_per_image[i] rows.  edges [n_bones,2] / mean_bones [n_bones] may be
    None (no bone-length test).  -> (keep_idx [P] i32: per image its kept rows then -1,
    keep_count [n_images] i32, valid [P] bool) -- all on the GPU, no host sync."""
    require_cuda(poses3d, poses2d, boxes)
    P, A, J, _ = poses3d.shape
    dev = poses3d.device
    n_images = len(n_per_image)
    counts = [int(x) for x in n_per_image]
    if sum(counts) != P:
        raise ValueError('n_per_image does not add up to the number of poses')
    row_start = torch.tensor([0] + list(torch.tensor(counts).cumsum(0).tolist()) if counts else [0],
                             dtype=torch.int32, device=dev)
    sq = [c * c for c in counts]
    sim_off = torch.tensor([sum(sq[:i]) for i in range(n_images)], dtype=torch.int32, device=dev)
    max_n = max(counts) if counts else 0
    lib = _lib.load()
    ws_bytes = lib.mtr_filter_poses_workspace_bytes(P, J, max_n)
    ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.float64, device=dev)
    valid = torch.zeros(P, dtype=torch.uint8, device=dev)
    keep_idx = torch.full((P,), -1, dtype=torch.int32, device=dev)
    keep_count = torch.zeros(n_images, dtype=torch.int32, device=dev)
    if edges is not None and len(edges):
        e = torch.as_tensor(edges, dtype=torch.int32, device=dev).contiguous()
        mb = torch.as_tensor(mean_bones, dtype=torch.float32, device=dev).contiguous()
        n_bones = e.shape[0]
    else:
        e = mb = None
        n_bones = 0
    fp = _lib.FilterParams(0.1, 3.0, 300.0, 200.0, 0.5, 300.0, 0.4, int(max_output),
                           1 if unbiased else 0, 1 if order == 'score' else 0)
    p3 = poses3d.float().contiguous()
    p2 = poses2d.float().contiguous()
    bx = boxes.float().contiguous()
    check(lib.mtr_filter_poses(_ptr(p3), _ptr(p2), _ptr(bx), _ptr(row_start), _ptr(sim_off), n_images,
                               P, A, J, _ptr(e) if e is not None else None,
                               _ptr(mb) if mb is not None else None, n_bones,
                               int(n_joints or J), ctypes.byref(fp), _ptr(ws), ws.numel() * 8, max_n,
                               _ptr(valid), _ptr(keep_idx), _ptr(keep_count),
                               current_stream_ptr(dev)), 'mtr_filter_poses')
    return keep_idx, keep_count, valid.bool()


# ------------------------------------------------------------------------------------------------
# K10: bias + activation epilogue for the backbone's inference copy (backbones.fold_batchnorm)

ACT_CODES = {None: 0, 'none': 0, 'relu': 1, 'silu': 2, 'hardswish': 3}


def bias_act_(y, bias, act, residual=None):
    """In place: y[b, c, ...] = act(y[b, c, ...] + bias[c]) (+ residual) on an NCHW-contiguous
    activation (f32 / f16 / bf16), one HBM pass instead of PyTorch-ROCm's bias-add, activation and
    skip-connection kernels."""
    require_cuda(y, bias)
    if not y.is_contiguous():
        raise ValueError('bias_act_ needs an NCHW-contiguous tensor')
    if residual is not None:
        if residual.shape != y.shape or residual.dtype != y.dtype or not residual.is_contiguous():
            raise ValueError('residual must match y in shape, dtype and layout')
    B, C = y.shape[0], y.shape[1]
    hw = y.numel() // max(B * C, 1)
    check(_lib.load().mtr_bias_act_nchw(_ptr(y), dtype_code(y.dtype), _ptr(bias.contiguous().float()),
                                        None if residual is None else _ptr(residual), ACT_CODES[act],
                                        B, C, hw, current_stream_ptr(y.device)),
          'mtr_bias_act_nchw')
    return y


def bias_act_rowmean_(y, bias, act):
    """bias_act_ + the mean over H*W of every (b, c) row of the result, [B, C] f32, from the same pass
    (what a squeeze-excite block behind the convolution starts with)."""
    require_cuda(y, bias)
    if not y.is_contiguous():
        raise ValueError('bias_act_rowmean_ needs an NCHW-contiguous tensor')
    B, C = y.shape[0], y.shape[1]
    hw = y.numel() // max(B * C, 1)
    mean = torch.empty(B, C, device=y.device, dtype=torch.float32)
    check(_lib.load().mtr_bias_act_rowmean_nchw(_ptr(y), dtype_code(y.dtype), _ptr(bias.contiguous().float()),
                                                ACT_CODES[act], B, C, hw, _ptr(mean),
                                                current_stream_ptr(y.device)),
          'mtr_bias_act_rowmean_nchw')
    return y, mean


def depthwise3x3_bias_act(x, weight, bias, act, stride, pad, want_mean=False):
    """K11: y = act(depthwise_conv3x3(x, weight) + bias) in one pass (+ the [B, C] f32 mean of y over
    H*W if want_mean).  x NCHW-contiguous f32 / f16 / bf16, weight [C, 1, 3, 3] or [C, 3, 3].
    pad: one int (every side) or (left, right, top, bottom) like torch.nn.ZeroPad2d -- the explicit
    padding in front of the reference's stride-2 layers, folded into the kernel."""
    require_cuda(x, weight, bias)
    if not x.is_contiguous():
        raise ValueError('depthwise3x3_bias_act needs an NCHW-contiguous tensor')
    if weight.numel() != x.shape[1] * 9:
        raise ValueError(f'depthwise3x3_bias_act needs a [C, 3, 3] weight, got {tuple(weight.shape)}')
    B, C, H, W = x.shape
    pl, pr, pt, pb = (pad,) * 4 if isinstance(pad, int) else tuple(int(p) for p in pad)
    OH, OW = (H + pt + pb - 3) // stride + 1, (W + pl + pr - 3) // stride + 1
    y = torch.empty(B, C, OH, OW, device=x.device, dtype=x.dtype)
    mean = torch.empty(B, C, device=x.device, dtype=torch.float32) if want_mean else None
    check(_lib.load().mtr_depthwise3x3_bias_act_padded(
        _ptr(x), dtype_code(x.dtype), _ptr(weight.contiguous().float()), _ptr(bias.contiguous().float()),
        ACT_CODES[act], B, C, H, W, int(stride), pt, pl, pb, pr, _ptr(y), None if mean is None else _ptr(mean),
        current_stream_ptr(x.device)), 'mtr_depthwise3x3_bias_act_padded')
    return (y, mean) if want_mean else y


# K18: the stride-1, padding-1 depthwise 3x3 layer on register blocks (csrc/depthwise3x3_blocks.hip)

def k11_takes_block_kernel(H, W):
    """Whether K11 (depthwise3x3_bias_act at stride 1, padding 1, on a 16-byte aligned x of fewer than 2^24
    planes) runs an [.., H, W] plane on its stride-1 block kernel instead of its generic kernel: launch_depthwise's
    condition in csrc/depthwise.hip, restated.  W / 4 and H / 4 powers of two, at most 16 blocks per row and 64
    per plane."""
    if H <= 0 or W <= 0 or H % 4 or W % 4:
        return False
    bw, bh = W // 4, H // 4
    if bw & (bw - 1) or bh & (bh - 1):
        return False
    return bw <= 16 and bw * bh <= 64


def depthwise3x3_blocks_supported(dtype, H, W, stride=1, pad=1, data_ptr=0):
    """Whether K18 takes a depthwise 3x3 layer on [.., H, W] planes of `dtype`: stride 1, zero padding 1 on all four
    sides (pad: an int or (left, right, top, bottom) like torch.nn.ZeroPad2d), W a multiple of 4 up to 128, H up to
    128, f32 / f16 / bf16, and -- where the tensor's data_ptr() is given -- a 16-byte aligned base.  Host only; the
    rules of mtr_depthwise3x3_blocks_supported, restated (a test holds the two together)."""
    pl, pr, pt, pb = (pad,) * 4 if isinstance(pad, int) else tuple(int(p) for p in pad)
    return (dtype in (torch.float32, torch.float16, torch.bfloat16) and stride == 1
            and (pl, pr, pt, pb) == (1, 1, 1, 1) and 1 <= H <= 128 and 4 <= W <= 128 and W % 4 == 0
            and data_ptr % 16 == 0)


def depthwise3x3_blocks_plan(dtype, H, W):
    """The block shape (4 or 8 columns of a lane's 4-row block) K18's own choice resolves to for [.., H, W] planes of
    `dtype`, or None where the kernel does not take them.  Host only (mtr_depthwise3x3_blocks_supported)."""
    import ctypes
    cols = ctypes.c_int(0)
    rc = _lib.load().mtr_depthwise3x3_blocks_supported(dtype_code(dtype), int(H), int(W), 1, 1, 1, 1, 1,
                                                       ctypes.addressof(cols))
    return cols.value if rc == 0 else None


def depthwise3x3_blocks_bias_act(x, weight, bias, act, want_mean=False, block_cols=None):
    """K18: y = act(depthwise_conv3x3(x, weight) + bias) at stride 1 and zero padding 1 in one pass over register
    blocks (+ the [B, C] f32 mean of y over H*W if want_mean), with the bits of depthwise3x3_bias_act's generic
    kernel for y and the mean.  x NCHW-contiguous f32 / f16 / bf16, 16-byte aligned, W % 4 == 0, H and W at most
    128; weight [C, 1, 3, 3] or [C, 3, 3].  block_cols: None the library's choice, 4 or 8 (f16 / bf16 with
    W % 8 == 0) columns of a lane's 4-row block; the bits do not depend on it.  What the kernel does not take
    raises (depthwise3x3_blocks_supported asks first); there is no fallback in here."""
    require_cuda(x, weight, bias)
    if not x.is_contiguous():
        raise ValueError('depthwise3x3_blocks_bias_act needs an NCHW-contiguous tensor')
    if weight.numel() != x.shape[1] * 9:
        raise ValueError(f'depthwise3x3_blocks_bias_act needs a [C, 3, 3] weight, got {tuple(weight.shape)}')
    if block_cols not in (None, 4, 8):
        raise ValueError(f'depthwise3x3_blocks_bias_act: block_cols must be None, 4 or 8, got {block_cols}')
    B, C, H, W = x.shape
    y = torch.empty(B, C, H, W, device=x.device, dtype=x.dtype)
    mean = torch.empty(B, C, device=x.device, dtype=torch.float32) if want_mean else None
    check(_lib.load().mtr_depthwise3x3_blocks_bias_act_opts(
        _ptr(x), dtype_code(x.dtype), _ptr(weight.contiguous().float()), _ptr(bias.contiguous().float()),
        ACT_CODES[act], B, C, H, W, _ptr(y), None if mean is None else _ptr(mean),
        current_stream_ptr(x.device), int(block_cols or 0)), 'mtr_depthwise3x3_blocks_bias_act_opts')
    return (y, mean) if want_mean else y


def depthwise5x5_supported(H, W, pad):
    """Whether K15 takes an [.., H, W] plane with padding `pad` (an int or (left, right, top, bottom)): the
    padded plane is staged through LDS and may be at most 112 x 112 (csrc/depthwise5x5.hip)."""
    pl, pr, pt, pb = (pad,) * 4 if isinstance(pad, int) else tuple(int(p) for p in pad)
    return H + pt + pb <= 112 and W + pl + pr <= 112


def depthwise5x5_bias_act(x, weight, bias, act, stride, pad, want_mean=False):
    """K15: y = act(depthwise_conv5x5(x, weight) + bias) in one pass (+ the [B, C] f32 mean of y over
    H*W if want_mean).  x NCHW-contiguous f32 / f16 / bf16, weight [C, 1, 5, 5] or [C, 5, 5].
    pad: one int (every side, 0..2) or (left, right, top, bottom) like torch.nn.ZeroPad2d (left / top 0..2,
    right / bottom 0..3).  A function of its own beside depthwise3x3_bias_act: the 3x3 layers never pass here
    and the 5x5 layers never pass there."""
    require_cuda(x, weight, bias)
    if not x.is_contiguous():
        raise ValueError('depthwise5x5_bias_act needs an NCHW-contiguous tensor')
    if weight.numel() != x.shape[1] * 25:
        raise ValueError(f'depthwise5x5_bias_act needs a [C, 5, 5] weight, got {tuple(weight.shape)}')
    B, C, H, W = x.shape
    pl, pr, pt, pb = (pad,) * 4 if isinstance(pad, int) else tuple(int(p) for p in pad)
    OH, OW = (H + pt + pb - 5) // stride + 1, (W + pl + pr - 5) // stride + 1
    y = torch.empty(B, C, max(OH, 0), max(OW, 0), device=x.device, dtype=x.dtype)
    mean = torch.empty(B, C, device=x.device, dtype=torch.float32) if want_mean else None
    check(_lib.load().mtr_depthwise5x5_bias_act_padded(
        _ptr(x), dtype_code(x.dtype), _ptr(weight.contiguous().float()), _ptr(bias.contiguous().float()),
        ACT_CODES[act], B, C, H, W, int(stride), pt, pl, pb, pr, _ptr(y), None if mean is None else _ptr(mean),
        current_stream_ptr(x.device)), 'mtr_depthwise5x5_bias_act_padded')
    return (y, mean) if want_mean else y


# K12: the squeeze-excite gate of an MBConv block (csrc/se.hip)

SE_GATE_CODES = {'sigmoid': 0, 'hardsigmoid': 1}


def se_gate(mean, w1, b1, w2, b2, act, gate_fn, out=None, w2t=None, config=-1):
    """gate [B, C] f32 = gate_fn(w2 . act(w1 . mean + b1) + b2) in one launch: the squeeze-excite block
    of an MBConv from the [B, C] f32 channel mean K10 / K11 emit (instead of PyTorch-ROCm's fc1 GEMM,
    bias, activation, fc2 GEMM, bias and gate kernels).  w1 [S, C] (or the [S, C, 1, 1] conv weight),
    w2 [C, S], b1 [S], b2 [C]; all f32.  act: a key of ACT_CODES, gate_fn: 'sigmoid' / 'hardsigmoid'.
    w2t: w2 transposed to [S, C] f32 contiguous (made once from a constant weight), read in place of w2 with
    contiguous loads: the same bits.  config: -1 the library's choice, 0 .. 3 a forced workgroup split."""
    require_cuda(mean, w1, b1, w2, b2, w2t)
    B, C = mean.shape[0], mean.shape[1]
    S = w1.shape[0]
    w1, w2 = w1.reshape(S, -1), w2.reshape(C, -1)
    if mean.dtype != torch.float32 or mean.numel() != B * C or w1.shape[1] != C or w2.shape[1] != S:
        raise ValueError('se_gate: mean [B, C] f32, w1 [S, C], w2 [C, S]')
    if w2t is not None:
        if w2t.shape != (S, C) or w2t.dtype != torch.float32 or not w2t.is_contiguous():
            raise ValueError('se_gate: w2t must be [S, C] f32, contiguous')
        w2 = w2t
    tensors = [t.contiguous().float() for t in (mean, w1, b1, w2, b2)]
    if out is None:
        out = torch.empty(B, C, device=mean.device, dtype=torch.float32)
    check(_lib.load().mtr_se_gate_opts(*(_ptr(t) for t in tensors), ACT_CODES[act], SE_GATE_CODES[gate_fn], B, C,
                                       S, _ptr(out), current_stream_ptr(mean.device),
                                       0 if w2t is None else 1, int(config)), 'mtr_se_gate_opts')
    return out


def _residual_and_out(fn, x, shape, residual, out, hw='H, W'):
    """What the convolution wrappers below ask of a skip connection and of a caller's `out`: `shape` (the output's),
    x's dtype, contiguous.  -> `out`, allocated here when None.  `fn` and `hw` go into the error text."""
    for name, t in (('residual', residual), ('out', out)):
        if t is not None and (t.shape != shape or t.dtype != x.dtype or not t.is_contiguous()):
            raise ValueError(f'{fn}: {name} must be [B, Cout, {hw}] like the output, contiguous')
    return torch.empty(shape, device=x.device, dtype=x.dtype) if out is None else out


# K13: 1x1 convolution as one f32 MFMA GEMM with the K10 epilogue (csrc/conv1x1.hip)

def conv1x1_supported(x, weight):
    """Whether mtr_conv1x1_bias_act takes this input: f32, NCHW-contiguous, 16-byte aligned, H*W and
    Cin multiples of 4 (its MTR_E_DTYPE / MTR_E_SHAPE / MTR_E_ALIGN rules, checked without a call)."""
    if x.dim() != 4 or x.dtype != torch.float32 or weight.dtype != torch.float32 or not x.is_contiguous():
        return False
    K, HW = x.shape[1], x.shape[2] * x.shape[3]
    return (weight.numel() == weight.shape[0] * K and HW % 4 == 0 and K % 4 == 0
            and x.data_ptr() % 16 == 0 and weight.data_ptr() % 16 == 0
            and x.shape[0] * HW < 2 ** 31 and K * HW < 2 ** 31 and weight.shape[0] * HW < 2 ** 31)


CONV1X1_CONFIGS = {'auto': -1, 'wide': 0, 'square': 1, 'tall': 2, 'deepk': 3, 'stream': 4, 'deep64': 5}


def _conv1x1_plan(entry, configs, M, K, HW, B, config):
    """conv1x1_plan and conv1x1_16_plan: the plan query `entry` of the library, its configuration code as a name of
    `configs`."""
    plan = (ctypes.c_int * 4)()
    check(getattr(_lib.load(), entry)(M, K, HW, B, configs[config], ctypes.addressof(plan)), entry)
    names = {v: k for k, v in configs.items()}
    return names[plan[0]], plan[1], plan[2], plan[3]


def conv1x1_plan(M, K, HW, B, config='auto'):
    """(configuration name, waves along the channels, channels per workgroup, columns per workgroup) K13 runs a
    shape with: the library's own choice, or what a forced `config` resolves to ('stream' on a shape whose weight does
    not fit LDS: 'tall').  Host only."""
    return _conv1x1_plan('mtr_conv1x1_plan', CONV1X1_CONFIGS, M, K, HW, B, config)


def conv1x1_bias_act(x, w, bias, act, gate=None, residual=None, out=None, config='auto', in_bias=None, in_act=None):
    """y = act(conv1x1(x * gate[:, :, None, None], w) + bias) (+ residual) in one launch on the current
    stream: x [B, K, H, W] f32 NCHW-contiguous, w [M, K] (or the [M, K, 1, 1] conv weight), bias [M],
    gate [B, K] f32 or None, residual [B, M, H, W] or None.  Stride 1, no padding; an f32 MFMA GEMM
    in a fixed k order (the same bits on every call and graph replay, and for every `config`: a key of
    CONV1X1_CONFIGS, 'auto' the library's own choice).
    in_bias [K] f32 (with in_act, a key of ACT_CODES): x comes from a convolution whose epilogue was left out, and
    every element enters the GEMM as in_act(x + in_bias[k]) (then * gate) -- the bits of
    conv1x1_bias_act(bias_act_(x, in_bias, in_act), ...) without that pass over x, which stays untouched."""
    require_cuda(x, w, bias, gate, residual, in_bias)
    B, K, H, W = x.shape
    M = w.shape[0]
    w = w.reshape(M, -1)
    if w.shape[1] != K:
        raise ValueError(f'conv1x1_bias_act: weight has {w.shape[1]} input channels, x has {K}')
    if gate is not None and (gate.dtype != torch.float32 or gate.numel() != B * K):
        raise ValueError('conv1x1_bias_act: gate must be [B, Cin] f32')
    if in_bias is None and in_act is not None:
        raise ValueError('conv1x1_bias_act: in_act needs in_bias')
    if in_bias is not None and (in_bias.dtype != torch.float32 or in_bias.numel() != K):
        raise ValueError('conv1x1_bias_act: in_bias must be [Cin] f32')
    out = _residual_and_out('conv1x1_bias_act', x, (B, M, H, W), residual, out)
    check(_lib.load().mtr_conv1x1_bias_act_pre(
        _ptr(x), dtype_code(x.dtype), _ptr(w.contiguous()), _ptr(bias.contiguous().float()),
        None if in_bias is None else _ptr(in_bias.contiguous()), ACT_CODES[in_act],
        None if gate is None else _ptr(gate.contiguous()), None if residual is None else _ptr(residual),
        ACT_CODES[act], B, M, K, H * W, _ptr(out), current_stream_ptr(x.device), CONV1X1_CONFIGS[config]),
        'mtr_conv1x1_bias_act_pre')
    return out


# K13h: the same for f16 / bf16 tensors, one 16-bit MFMA GEMM (csrc/conv1x1_16.hip)

def conv1x1_16_supported(x, weight):
    """Whether mtr_conv1x1_bias_act16 takes this input: f16 or bf16 x and weight of one dtype, NCHW-contiguous,
    16-byte aligned, H*W and Cin multiples of 8 (its MTR_E_DTYPE / MTR_E_SHAPE / MTR_E_ALIGN rules, checked
    without a call)."""
    if x.dim() != 4 or x.dtype not in (torch.float16, torch.bfloat16) or weight.dtype != x.dtype \
            or not x.is_contiguous() or not weight.is_contiguous():
        return False
    K, HW = x.shape[1], x.shape[2] * x.shape[3]
    return (weight.numel() == weight.shape[0] * K and HW % 8 == 0 and K % 8 == 0
            and x.data_ptr() % 16 == 0 and weight.data_ptr() % 16 == 0
            and x.shape[0] * HW < 2 ** 31 and K * HW < 2 ** 31 and weight.shape[0] * HW < 2 ** 31)


CONV1X1_16_CONFIGS = {'auto': -1, 'tall': 0, 'square': 1, 'deepk': 2}


def conv1x1_16_plan(M, K, HW, B, config='auto'):
    """(configuration name, waves along the channels, channels per workgroup, columns per workgroup) K13h runs a
    shape with: the library's own choice, or what a forced `config` resolves to.  Host only."""
    return _conv1x1_plan('mtr_conv1x1_plan16', CONV1X1_16_CONFIGS, M, K, HW, B, config)


def conv1x1_bias_act16(x, w, bias, act, gate=None, residual=None, out=None, config='auto'):
    """y = act(conv1x1(x * gate.to(x.dtype)[:, :, None, None], w) + bias) (+ residual) in one launch on the
    current stream, for f16 / bf16: x [B, K, H, W] NCHW-contiguous, w [M, K] (or the [M, K, 1, 1] conv weight)
    in x's dtype, bias [M] f32, gate [B, K] f32 or None, residual [B, M, H, W] in x's dtype or None.  Stride 1,
    no padding; f32 accumulation in a fixed k order, rounded to x's dtype once (the same bits on every call
    and graph replay, and for every `config`: a key of CONV1X1_16_CONFIGS, 'auto' the library's own choice)."""
    require_cuda(x, w, bias, gate, residual)
    code = CONV1X1_16_CONFIGS[config]
    B, K, H, W = x.shape
    M = w.shape[0]
    w = w.reshape(M, -1)
    if w.shape[1] != K:
        raise ValueError(f'conv1x1_bias_act16: weight has {w.shape[1]} input channels, x has {K}')
    if w.dtype != x.dtype:
        raise ValueError(f'conv1x1_bias_act16: weight is {w.dtype}, x is {x.dtype}')
    if gate is not None and (gate.dtype != torch.float32 or gate.numel() != B * K):
        raise ValueError('conv1x1_bias_act16: gate must be [B, Cin] f32')
    out = _residual_and_out('conv1x1_bias_act16', x, (B, M, H, W), residual, out)
    args = (_ptr(x), dtype_code(x.dtype), _ptr(w.contiguous()), _ptr(bias.contiguous().float()),
            None if gate is None else _ptr(gate.contiguous()), None if residual is None else _ptr(residual),
            ACT_CODES[act], B, M, K, H * W, _ptr(out), current_stream_ptr(x.device))
    if code < 0:  # today's call
        check(_lib.load().mtr_conv1x1_bias_act16(*args), 'mtr_conv1x1_bias_act16')
    else:
        check(_lib.load().mtr_conv1x1_bias_act16_opts(*args, code), 'mtr_conv1x1_bias_act16_opts')
    return out


# K14h: a dense 3x3 convolution of f16 / bf16 tensors as one implicit 16-bit MFMA GEMM (csrc/conv3x3_16.hip)

def pack_conv3x3_weight(weight):
    """The [Cout, Cin, 3, 3] convolution weight as mtr_conv3x3_bias_act16 takes it: [Cout, 3, 3, Cin], contiguous
    (the reduction runs over (ky, kx, ci) with ci innermost).  Plain torch; done once, at fold time."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError(f'pack_conv3x3_weight: expected [Cout, Cin, 3, 3], got {tuple(weight.shape)}')
    return weight.detach().permute(0, 2, 3, 1).contiguous()


def conv3x3_16_supported(x, weight, stride):
    """Whether mtr_conv3x3_bias_act16 takes this input: f16 or bf16 x and weight of one dtype, x NCHW-contiguous and
    16-byte aligned, stride 1 or 2, Cin a multiple of 8, the input and output widths multiples of 4, the input
    halo of a tile within LDS (its MTR_E_DTYPE / MTR_E_SHAPE / MTR_E_ALIGN rules, checked without a launch).
    `weight` is the convolution weight, [Cout, Cin, 3, 3] or packed [Cout, 3, 3, Cin]."""
    if x.dim() != 4 or weight.dim() != 4 or x.dtype not in (torch.float16, torch.bfloat16) \
            or weight.dtype != x.dtype or not x.is_contiguous() or x.data_ptr() % 16 or weight.data_ptr() % 16:
        return False
    B, K, H, W = x.shape
    if weight.numel() != weight.shape[0] * K * 9 or B >= 2 ** 16:
        return False
    return _lib.load().mtr_conv3x3_16_lds_bytes(B, K, weight.shape[0], H, W, int(stride)) > 0


def conv3x3_bias_act16(x, w_packed, bias, act, stride, residual=None, out=None):
    """y = act(conv3x3(x, w, stride, padding 1) + bias) (+ residual) in one launch on the current stream, for
    f16 / bf16: x [B, Cin, H, W] NCHW-contiguous, w_packed [Cout, 3, 3, Cin] (pack_conv3x3_weight) in x's dtype,
    bias [Cout] f32, residual [B, Cout, Ho, Wo] in x's dtype or None.  f32 accumulation in a fixed k order,
    rounded to x's dtype once (the same bits on every call and graph replay)."""
    require_cuda(x, w_packed, bias, residual)
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError('conv3x3_bias_act16: x must be [B, Cin, H, W], NCHW-contiguous')
    B, K, H, W = x.shape
    M = w_packed.shape[0]
    if w_packed.dim() != 4 or tuple(w_packed.shape[1:]) != (3, 3, K) or not w_packed.is_contiguous():
        raise ValueError(f'conv3x3_bias_act16: the weight must be packed [Cout, 3, 3, {K}] and contiguous, '
                         f'got {tuple(w_packed.shape)}')
    if w_packed.dtype != x.dtype:
        raise ValueError(f'conv3x3_bias_act16: weight is {w_packed.dtype}, x is {x.dtype}')
    if stride not in (1, 2):
        raise ValueError(f'conv3x3_bias_act16: stride must be 1 or 2, got {stride}')
    if bias.numel() != M:
        raise ValueError(f'conv3x3_bias_act16: bias has {bias.numel()} elements, expected {M}')
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = _residual_and_out('conv3x3_bias_act16', x, (B, M, Ho, Wo), residual, out, hw='Ho, Wo')
    check(_lib.load().mtr_conv3x3_bias_act16(
        _ptr(x), dtype_code(x.dtype), _ptr(w_packed), _ptr(bias.contiguous().float()),
        None if residual is None else _ptr(residual), ACT_CODES[act], B, K, M, H, W, int(stride), _ptr(out),
        current_stream_ptr(x.device)), 'mtr_conv3x3_bias_act16')
    return out


# K16h: a FusedMBConv block of f16 / bf16 tensors -- K14h's 3x3 expand and K13h's 1x1 project -- as one launch
# (csrc/fused_mbconv16.hip)

def fused_mbconv16_supported(x, w3_packed, w1, stride):
    """Whether mtr_fused_mbconv16 takes this input: f16 or bf16 x and weights of one dtype, x NCHW-contiguous and
    16-byte aligned, stride 1 or 2, Cin and Cmid multiples of 8, the input and output widths multiples of 4,
    Cout <= 128, the input halo of a tile and one chunk of the intermediate within LDS (its MTR_E_DTYPE /
    MTR_E_SHAPE / MTR_E_ALIGN rules, checked without a launch).  `w3_packed` is the expand's weight packed
    [Cmid, 3, 3, Cin] (pack_conv3x3_weight), `w1` the project's, [Cout, Cmid] or [Cout, Cmid, 1, 1]."""
    if x.dim() != 4 or w3_packed.dim() != 4 or x.dtype not in (torch.float16, torch.bfloat16) \
            or w3_packed.dtype != x.dtype or w1.dtype != x.dtype or not x.is_contiguous() \
            or not w3_packed.is_contiguous() or not w1.is_contiguous() \
            or x.data_ptr() % 16 or w3_packed.data_ptr() % 16 or w1.data_ptr() % 16:
        return False
    B, K, H, W = x.shape
    Cmid, Cout = w3_packed.shape[0], w1.shape[0]
    if tuple(w3_packed.shape[1:]) != (3, 3, K) or w1.numel() != Cout * Cmid or B >= 2 ** 16:
        return False
    return _lib.load().mtr_fused_mbconv16_lds_bytes(B, K, Cmid, Cout, H, W, int(stride)) > 0


def fused_mbconv16(x, w3_packed, bias3, act, stride, w1, bias1, residual=None, out=None):
    """y = conv1x1(act(conv3x3(x, w3, stride, padding 1) + bias3), w1) + bias1 (+ residual) in one launch on the
    current stream, for f16 / bf16: x [B, Cin, H, W] NCHW-contiguous, w3_packed [Cmid, 3, 3, Cin]
    (pack_conv3x3_weight) and w1 [Cout, Cmid] (or the [Cout, Cmid, 1, 1] conv weight) in x's dtype, bias3 [Cmid]
    and bias1 [Cout] f32, residual [B, Cout, Ho, Wo] in x's dtype or None (stride 1 and Cout == Cin only; it may be
    x itself).  The intermediate stays on the chip, rounded to x's dtype once; the result has the bits of
    conv3x3_bias_act16 followed by conv1x1_bias_act16 (the same on every call and graph replay)."""
    require_cuda(x, w3_packed, bias3, w1, bias1, residual)
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError('fused_mbconv16: x must be [B, Cin, H, W], NCHW-contiguous')
    B, K, H, W = x.shape
    Cmid = w3_packed.shape[0]
    if w3_packed.dim() != 4 or tuple(w3_packed.shape[1:]) != (3, 3, K) or not w3_packed.is_contiguous():
        raise ValueError(f'fused_mbconv16: the 3x3 weight must be packed [Cmid, 3, 3, {K}] and contiguous, '
                         f'got {tuple(w3_packed.shape)}')
    M = w1.shape[0]
    w1 = w1.reshape(M, -1)
    if w1.shape[1] != Cmid:
        raise ValueError(f'fused_mbconv16: the 1x1 weight has {w1.shape[1]} input channels, the 3x3 weight '
                         f'{Cmid} output channels')
    if w3_packed.dtype != x.dtype or w1.dtype != x.dtype:
        raise ValueError(f'fused_mbconv16: weights are {w3_packed.dtype} and {w1.dtype}, x is {x.dtype}')
    if stride not in (1, 2):
        raise ValueError(f'fused_mbconv16: stride must be 1 or 2, got {stride}')
    if bias3.numel() != Cmid or bias1.numel() != M:
        raise ValueError(f'fused_mbconv16: biases have {bias3.numel()} and {bias1.numel()} elements, expected '
                         f'{Cmid} and {M}')
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    if residual is not None and (stride != 1 or M != K):
        raise ValueError('fused_mbconv16: a residual needs stride 1 and Cout == Cin')
    out = _residual_and_out('fused_mbconv16', x, (B, M, Ho, Wo), residual, out, hw='Ho, Wo')
    check(_lib.load().mtr_fused_mbconv16(
        _ptr(x), dtype_code(x.dtype), _ptr(w3_packed), _ptr(bias3.contiguous().float()), ACT_CODES[act],
        _ptr(w1.contiguous()), _ptr(bias1.contiguous().float()), None if residual is None else _ptr(residual),
        B, K, Cmid, M, H, W, int(stride), _ptr(out), current_stream_ptr(x.device)), 'mtr_fused_mbconv16')
    return out


# K25h: the 1x1 expand of an MBConv block of f16 / bf16 tensors (K13h) and the depthwise 3x3 stride-1 layer behind it
# (K11's block kernel) as one launch (csrc/expand_dw16.hip)

EXPAND_DW16_MAPPINGS = {'auto': -1, 'plain': 0, 'xcd': 1}


def _expand_dw16_supported(x, w1, query, *extra):
    """The tensor rules K25h, K26h and K27h share, then the C library's own shape query `query`(B, Cin, Cmid, H, W,
    *extra) > 0."""
    if x.dim() != 4 or x.dtype not in (torch.float16, torch.bfloat16) or w1.dtype != x.dtype \
            or not x.is_contiguous() or not w1.is_contiguous() or x.data_ptr() % 16 or w1.data_ptr() % 16:
        return False
    B, K, H, W = x.shape
    if w1.numel() != w1.shape[0] * K:
        return False
    return getattr(_lib.load(), query)(B, K, w1.shape[0], H, W, *extra) > 0


def _expand_dw16_check(name, x, w1, bias1, w_dw, bias_dw, stride=1, k=3):
    """The argument checks of the wrapper `name`, in their order -> (B, Cin, Cmid, H, W, w1 as [Cmid, Cin]).  `stride`
    is expand_depthwise16_tiles' and expand_depthwise16_k5's (the other two have none and leave the default): its
    refusal keeps its place, right behind x's.  `k`: the depthwise kernel size, 3 or expand_depthwise16_k5's 5."""
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f'{name}: x must be [B, Cin, H, W], NCHW-contiguous')
    if stride not in (1, 2):
        raise ValueError(f'{name}: stride must be 1 or 2, got {stride}')
    B, K, H, W = x.shape
    Cmid = w1.shape[0]
    w1 = w1.reshape(Cmid, -1)
    if w1.shape[1] != K:
        raise ValueError(f'{name}: the 1x1 weight has {w1.shape[1]} input channels, x has {K}')
    if w1.dtype != x.dtype:
        raise ValueError(f'{name}: the 1x1 weight is {w1.dtype}, x is {x.dtype}')
    if w_dw.numel() != Cmid * k * k:
        raise ValueError(f'{name}: the depthwise weight must be [{Cmid}, {k}, {k}], got {tuple(w_dw.shape)}')
    if bias1.numel() != Cmid or bias_dw.numel() != Cmid:
        raise ValueError(f'{name}: biases have {bias1.numel()} and {bias_dw.numel()} elements, expected {Cmid} each')
    return B, K, Cmid, H, W, w1


def _expand_dw16_run(name, entry, x, w1, bias1, act1, w_dw, bias_dw, act2, out, out_hw=lambda H, W: (H, W),
                     stride=None, k=3, want_mean=None, mapping=None):
    """The body of the wrapper `name` of the C entry `entry`: the checks above, `out` [B, Cmid, *out_hw(H, W)] and the
    mean, the call.  What an entry does not have stays None: `stride` (K25h, K26h), `want_mean` (K27h has no mean
    argument), `mapping` (K27h has no `entry`_opts, which the others take for a mapping other than 'auto')."""
    require_cuda(x, w1, bias1, w_dw, bias_dw, out)
    code = -1 if mapping is None else EXPAND_DW16_MAPPINGS[mapping]
    B, K, Cmid, H, W, w1 = _expand_dw16_check(name, x, w1, bias1, w_dw, bias_dw, 1 if stride is None else stride, k)
    out = _residual_and_out(name, x, (B, Cmid, *out_hw(H, W)), None, out)
    mean = torch.empty(B, Cmid, device=x.device, dtype=torch.float32) if want_mean else None
    args = (_ptr(x), dtype_code(x.dtype), _ptr(w1.contiguous()), _ptr(bias1.contiguous().float()), ACT_CODES[act1],
            _ptr(w_dw.contiguous().float()), _ptr(bias_dw.contiguous().float()), ACT_CODES[act2], B, K, Cmid, H, W,
            *(() if stride is None else (int(stride),)), _ptr(out),
            *(() if want_mean is None else (None if mean is None else _ptr(mean),)), current_stream_ptr(x.device))
    if code < 0:
        check(getattr(_lib.load(), entry)(*args), entry)
    else:
        check(getattr(_lib.load(), entry + '_opts')(*args, code), entry + '_opts')
    return (out, mean) if want_mean else out


def expand_depthwise16_supported(x, w1):
    """Whether mtr_expand_dw16 takes this input: f16 or bf16 x and 1x1 weight of one dtype, x NCHW-contiguous, both
    16-byte aligned, Cin a multiple of 8, an [.., H, W] plane K11 runs on its stride-1 block kernel
    (k11_takes_block_kernel) of at most 256 positions, fewer than 2^24 planes of output (its MTR_E_DTYPE /
    MTR_E_SHAPE / MTR_E_ALIGN rules, checked without a launch).  `w1` is the expand's weight, [Cmid, Cin] or
    [Cmid, Cin, 1, 1]."""
    return _expand_dw16_supported(x, w1, 'mtr_expand_dw16_lds_bytes')


def expand_depthwise16(x, w1, bias1, act1, w_dw, bias_dw, act2, want_mean=False, out=None, mapping='auto'):
    """y = act2(depthwise_conv3x3(act1(conv1x1(x, w1) + bias1), w_dw, stride 1, padding 1) + bias_dw) in one launch
    on the current stream (+ the [B, Cmid] f32 mean of y over H*W if want_mean), for f16 / bf16: x [B, Cin, H, W]
    NCHW-contiguous, w1 [Cmid, Cin] (or the [Cmid, Cin, 1, 1] conv weight) in x's dtype, bias1 [Cmid] f32, w_dw
    [Cmid, 1, 3, 3] or [Cmid, 3, 3] and bias_dw [Cmid] (taken as f32, as depthwise3x3_bias_act takes them).  The
    expanded activation stays on the chip, rounded to x's dtype once; y and the mean have the bits of
    conv1x1_bias_act16 followed by depthwise3x3_bias_act(.., 1, 1, want_mean=True) (the same on every call and graph
    replay, and for every `mapping`: a key of EXPAND_DW16_MAPPINGS).  What the kernel does not take raises
    (expand_depthwise16_supported asks first); there is no fallback in here."""
    return _expand_dw16_run('expand_depthwise16', 'mtr_expand_dw16', x, w1, bias1, act1, w_dw, bias_dw, act2, out,
                            want_mean=bool(want_mean), mapping=mapping)


# K26h: the same pair on the planes K11 runs on its generic kernel, 24x24 and 12x12 among them
# (csrc/expand_dw16_planes.hip)

def expand_depthwise16_planes_supported(x, w1):
    """Whether mtr_expand_dw16_planes takes this input: f16 or bf16 x and 1x1 weight of one dtype, x NCHW-contiguous,
    both 16-byte aligned, Cin a multiple of 8, an [.., H, W] plane with W % 4 == 0, H W % 8 == 0, H and W at most 32
    and H W at most 576 that K11 does NOT run on its stride-1 block kernel (k11_takes_block_kernel), fewer than 2^30
    planes of output (its MTR_E_DTYPE / MTR_E_SHAPE / MTR_E_ALIGN rules, checked without a launch).  `w1` is the
    expand's weight, [Cmid, Cin] or [Cmid, Cin, 1, 1]."""
    return _expand_dw16_supported(x, w1, 'mtr_expand_dw16_planes_lds_bytes')


def expand_depthwise16_planes(x, w1, bias1, act1, w_dw, bias_dw, act2, want_mean=False, out=None, mapping='auto'):
    """expand_depthwise16 for the planes it refuses (K26h): the same arguments and result, in one launch on the
    current stream.  y and the mean have the bits of conv1x1_bias_act16 followed by depthwise3x3_bias_act(.., 1, 1,
    want_mean=True) on such a plane -- K11's generic kernel, so also the bits of depthwise3x3_blocks_bias_act behind
    conv1x1_bias_act16 -- the same on every call and graph replay, and for every `mapping` (a key of
    EXPAND_DW16_MAPPINGS).  What the kernel does not take raises (expand_depthwise16_planes_supported asks first);
    there is no fallback in here."""
    return _expand_dw16_run('expand_depthwise16_planes', 'mtr_expand_dw16_planes', x, w1, bias1, act1, w_dw, bias_dw,
                            act2, out, want_mean=bool(want_mean), mapping=mapping)


# K27h: the same pair on large planes, stride 1 or 2, in bands of output rows and without a mean
# (csrc/expand_dw16_tiles.hip)

def expand_depthwise16_tiles_supported(x, w1, stride=1):
    """Whether mtr_expand_dw16_tiles takes this input: f16 or bf16 x and 1x1 weight of one dtype, x NCHW-contiguous,
    both 16-byte aligned, Cin a multiple of 8, H and W at most 128, fewer than 2^30 planes of output; at stride 1
    W % 4 == 0, H W % 8 == 0 and a plane K11 does NOT run on its stride-1 block kernel (k11_takes_block_kernel); at
    stride 2 H even and W % 8 == 0 (its MTR_E_DTYPE / MTR_E_SHAPE / MTR_E_ALIGN rules, checked without a launch).
    `w1` is the expand's weight, [Cmid, Cin] or [Cmid, Cin, 1, 1]."""
    return _expand_dw16_supported(x, w1, 'mtr_expand_dw16_tiles_lds_bytes', int(stride))


def expand_depthwise16_tiles(x, w1, bias1, act1, w_dw, bias_dw, act2, stride=1, out=None):
    """K27h: y = act2(depthwise_conv3x3(act1(conv1x1(x, w1) + bias1), w_dw, stride, padding 1) + bias_dw) in one launch
    on the current stream, the expanded activation kept in LDS band by band; no mean.  y [B, Cmid, H / stride,
    W / stride] has the bits of conv1x1_bias_act16 followed by depthwise3x3_bias_act(.., stride, 1) on a plane K11 runs
    on its generic kernel (at stride 1 also the bits of depthwise3x3_blocks_bias_act behind conv1x1_bias_act16), the
    same on every call and graph replay.  What the kernel does not take raises (expand_depthwise16_tiles_supported
    asks first); there is no fallback in here."""
    return _expand_dw16_run('expand_depthwise16_tiles', 'mtr_expand_dw16_tiles', x, w1, bias1, act1, w_dw, bias_dw,
                            act2, out, lambda H, W: (H // stride, W // stride), stride)


# K28h: the 1x1 expand and the depthwise 5x5 layer behind it (K15), stride 1 or 2, padding 2, with the mean
# (csrc/expand_dw16_k5.hip)

def expand_depthwise16_k5_supported(x, w1, stride=1):
    """Whether mtr_expand_dw16_k5 takes this input: f16 or bf16 x and 1x1 weight of one dtype, x NCHW-contiguous, both
    16-byte aligned, Cin a multiple of 8, stride 1 or 2, W % 4 == 0, H W % 8 == 0, an output row of a multiple of four
    elements, a padded plane of at most 112 x 112 (K15's bound), fewer than 2^30 planes of output, and the image of 32
    expanded channels inside 160 KiB of LDS -- 32x32 at stride 1 is, 64x64 is not (its MTR_E_DTYPE / MTR_E_SHAPE /
    MTR_E_ALIGN rules, checked without a launch).  `w1` is the expand's weight, [Cmid, Cin] or [Cmid, Cin, 1, 1]."""
    return _expand_dw16_supported(x, w1, 'mtr_expand_dw16_k5_lds_bytes', int(stride))


def expand_depthwise16_k5(x, w1, bias1, act1, w_dw, bias_dw, act2, stride=1, want_mean=False, out=None,
                          mapping='auto'):
    """K28h: y = act2(depthwise_conv5x5(act1(conv1x1(x, w1) + bias1), w_dw, stride, padding 2) + bias_dw) in one launch
    on the current stream (+ the [B, Cmid] f32 mean of y over its plane if want_mean), the expanded activation kept in
    LDS; w_dw [Cmid, 1, 5, 5] or [Cmid, 5, 5].  y [B, Cmid, (H - 1) // stride + 1, (W - 1) // stride + 1] and the mean
    have the bits of conv1x1_bias_act16 followed by depthwise5x5_bias_act(.., stride, 2, want_mean=True), the same on
    every call and graph replay, and for every `mapping` (a key of EXPAND_DW16_MAPPINGS).  What the kernel does not take
    raises (expand_depthwise16_k5_supported asks first); there is no fallback in here."""
    return _expand_dw16_run('expand_depthwise16_k5', 'mtr_expand_dw16_k5', x, w1, bias1, act1, w_dw, bias_dw, act2,
                            out, lambda H, W: ((H - 1) // stride + 1, (W - 1) // stride + 1), stride, 5,
                            bool(want_mean), mapping)


# K17: the backbone stem -- Preproc and the dense 3x3 stride-2 Cin = 3 convolution with the K10 epilogue -- as one
# launch (csrc/stem_conv.hip)

def _stem_layout(x):
    """MTR_NCHW for a contiguous [B, 3, H, W], MTR_NHWC for a channels_last view over interleaved [B, H, W, 3]
    memory, None for any other strides."""
    if x.dim() != 4:
        return None
    if x.is_contiguous():
        return _lib.MTR_NCHW
    B, C, H, W = x.shape
    sb, sc, sh, sw = x.stride()
    if C == 3 and (sc, sh, sw) == (1, 3 * W, 3) and (B == 1 or sb == 3 * H * W):
        return _lib.MTR_NHWC
    return None


def stem_conv_supported(x, weight):
    """Whether mtr_stem_conv3x3s2 takes this input: CUDA tensors, x [B, 3, H, W] f32 / f16 / bf16, contiguous or channels_last
    (interleaved [B, H, W, 3] memory), 16-byte aligned; weight OIHW [Cout, 3, 3, 3] contiguous, f32 / f16 / bf16,
    of x's dtype or 16-bit with an f32 x; H even, W % 8 == 0, Cout % 8 == 0, Cout <= 64 (its MTR_E_DTYPE /
    MTR_E_SHAPE / MTR_E_ALIGN rules, checked without a launch)."""
    if not (x.is_cuda and weight.is_cuda):
        return False
    if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape[1:]) != (3, 3, 3) or not weight.is_contiguous():
        return False
    ok = (torch.float32, torch.float16, torch.bfloat16)
    if weight.dtype not in ok or x.dtype not in ok or not (x.dtype == weight.dtype or x.dtype == torch.float32):
        return False
    if _stem_layout(x) is None or x.data_ptr() % 16 or weight.data_ptr() % weight.element_size():
        return False
    B, K, H, W = x.shape
    if B >= 2 ** 16:
        return False
    return _lib.load().mtr_stem_conv_lds_bytes(dtype_code(weight.dtype), B, K, weight.shape[0], H, W) > 0


def stem_conv_bias_act(x, weight, bias, act, preproc=False, out=None):
    """y = act(conv3x3(p, weight, stride 2, padding 1) + bias) in one launch on the current stream, where p is x, or
    with preproc=True torch's (x * 2 - 1).to(weight.dtype) (the padding ring is zero after it): x [B, 3, H, W],
    contiguous or channels_last, in the weight's dtype or f32; weight the OIHW [Cout, 3, 3, 3] convolution weight
    (f32, f16 or bf16); bias [Cout] f32.  The result is [B, Cout, H / 2, W / 2], NCHW-contiguous, in the weight's
    dtype: f32 accumulation in a fixed k order, rounded once (the same bits for either layout, on every call and
    graph replay)."""
    require_cuda(x, weight, bias, out)
    layout = _stem_layout(x)
    if layout is None:
        raise ValueError('stem_conv_bias_act: x must be [B, 3, H, W], contiguous or channels_last')
    B, K, H, W = x.shape
    M = weight.shape[0]
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (K, 3, 3) or not weight.is_contiguous():
        raise ValueError(f'stem_conv_bias_act: the weight must be [Cout, {K}, 3, 3] and contiguous, '
                         f'got {tuple(weight.shape)}')
    if bias.numel() != M:
        raise ValueError(f'stem_conv_bias_act: bias has {bias.numel()} elements, expected {M}')
    if out is None:
        out = torch.empty(B, M, H // 2, W // 2, device=x.device, dtype=weight.dtype)
    elif out.shape != (B, M, H // 2, W // 2) or out.dtype != weight.dtype or not out.is_contiguous():
        raise ValueError('stem_conv_bias_act: out must be [B, Cout, H / 2, W / 2] in the weight\'s dtype, contiguous')
    check(_lib.load().mtr_stem_conv3x3s2(
        _ptr(x), dtype_code(x.dtype), layout, _ptr(weight), _ptr(bias.contiguous().float()),
        dtype_code(weight.dtype), ACT_CODES[act], int(bool(preproc)), B, K, M, H, W, _ptr(out),
        current_stream_ptr(x.device)), 'mtr_stem_conv3x3s2')
    return out


# The f32 dense 3x3 kernels K19, K21 and K22: one body for their `_supported` predicates and one for their wrappers.
# Each names its C entry and its weight rule `fits(w, Cin)`; a wrapper also the words of the rule's refusal and the stride.

def _dense3x3_supported(x, w, fits, query):
    """CUDA f32 x [B, Cin, H, W], NCHW-contiguous, x and w 16-byte aligned, `fits(w, Cin)`, then the C library's own
    shape query `query`(B, Cin, Cout, H, W) > 0."""
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda or not w.is_cuda or not x.is_contiguous() \
            or x.data_ptr() % 16 or w.data_ptr() % 16:
        return False
    B, K, H, W = x.shape
    return bool(fits(w, K)) and getattr(_lib.load(), query)(B, K, w.shape[1], H, W) > 0


def _dense3x3_bias_act(fn, entry, stride, fits, wanted, x, w, bias, act, residual, out):
    """The wrapper `fn` of the C entry `entry`: the checks in their order, `out` [B, Cout, H / stride, W / stride], the
    call.  `wanted` is the packed weight in the words of the refusal, with {K} for Cin.  A wrapper whose weight is f32
    names x's dtype together with the weight's; one whose weight is bf16 asks f32 of x at once and shows the weight's
    dtype behind its shape."""
    require_cuda(x, w, bias, residual)
    w_f32 = 'bf16' not in wanted
    if x.dim() != 4 or not x.is_contiguous() or not (w_f32 or x.dtype == torch.float32):
        raise ValueError(f'{fn}: x must be [B, Cin, H, W]{"" if w_f32 else " f32"}, NCHW-contiguous')
    if w_f32 and (x.dtype != torch.float32 or w.dtype != torch.float32):
        raise ValueError(f'{fn}: x and the weight must be f32, got {x.dtype} and {w.dtype}')
    B, K, H, W = x.shape
    if not fits(w, K):
        raise ValueError(f'{fn}: the weight must be {wanted.format(K=K)}, got {tuple(w.shape)}'
                         + ('' if w_f32 else f' {w.dtype}'))
    M = w.shape[1]
    if bias.numel() != M:
        raise ValueError(f'{fn}: bias has {bias.numel()} elements, expected {M}')
    if stride == 2 and (H % 2 or W % 2):
        raise ValueError(f'{fn}: H and W must be even, got {H} x {W}')
    out = _residual_and_out(fn, x, (B, M, H // stride, W // stride), residual, out,
                            hw='H, W' if stride == 1 else 'H / 2, W / 2')
    for t, name in ((x, 'x'), (residual, 'residual')):
        if t is not None and t.numel() and out.numel() and t.data_ptr() < out.data_ptr() + out.numel() * 4 \
                and out.data_ptr() < t.data_ptr() + t.numel() * 4:
            raise ValueError(f'{fn}: out must not overlap {name}')
    check(getattr(_lib.load(), entry)(
        _ptr(x), _ptr(w), _ptr(bias.contiguous().float()), None if residual is None else _ptr(residual),
        ACT_CODES[act], B, K, M, H, W, _ptr(out), current_stream_ptr(x.device)), entry)
    return out


# K19: a dense 3x3 stride-1 convolution of f32 tensors as Winograd F(2x2, 3x3) on the f32 MFMA, with the K10 epilogue
# (csrc/conv3x3_winograd.hip)

_WINOGRAD_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def pack_conv3x3_winograd_weight(weight):
    """The [Cout, Cin, 3, 3] f32 convolution weight as mtr_conv3x3_winograd_bias_act takes it: U = G g G^T per
    (Cout, Cin) pair, computed in fp64 and rounded to f32 once, laid out [16, Cout, Cin] (xi = 4 i + j), contiguous.
    Plain torch; done once per weight."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3):
        raise ValueError(f'pack_conv3x3_winograd_weight: expected [Cout, Cin, 3, 3], got {tuple(weight.shape)}')
    if weight.dtype != torch.float32:
        raise ValueError(f'pack_conv3x3_winograd_weight: expected an f32 weight, got {weight.dtype}')
    g = weight.detach().double()
    G = torch.tensor(_WINOGRAD_G, dtype=torch.float64, device=g.device)
    u = torch.einsum('ik,mckl,jl->ijmc', G, g, G)   # [4, 4, Cout, Cin]
    return u.reshape(16, weight.shape[0], weight.shape[1]).float().contiguous()


def _conv3x3_winograd_weight_fits(w_u, K):
    return w_u.dim() == 3 and w_u.dtype == torch.float32 and w_u.shape[0] == 16 and w_u.shape[2] == K \
        and w_u.is_contiguous()


def conv3x3_winograd_supported(x, w_u):
    """Whether mtr_conv3x3_winograd_bias_act takes this input: CUDA f32 x [B, Cin, H, W], NCHW-contiguous and 16-byte
    aligned, w_u [16, Cout, Cin] f32 contiguous (pack_conv3x3_winograd_weight), H even, W and Cin multiples of 4 (its
    MTR_E_SHAPE / MTR_E_ALIGN rules, checked without a launch)."""
    return _dense3x3_supported(x, w_u, _conv3x3_winograd_weight_fits, 'mtr_conv3x3_winograd_lds_bytes')


def conv3x3_winograd_bias_act(x, w_u, bias, act, residual=None, out=None):
    """y = act(conv3x3(x, w, stride 1, padding 1) + bias) (+ residual) in one launch on the current stream, for f32:
    x [B, Cin, H, W] NCHW-contiguous, w_u [16, Cout, Cin] (pack_conv3x3_winograd_weight), bias [Cout] f32, residual
    [B, Cout, H, W] f32 or None (it may be x).  Winograd F(2x2, 3x3) with f32 MFMA chains in a fixed order: the same
    bits on every call and graph replay."""
    return _dense3x3_bias_act('conv3x3_winograd_bias_act', 'mtr_conv3x3_winograd_bias_act', 1,
                              _conv3x3_winograd_weight_fits, 'transformed [16, Cout, {K}] and contiguous',
                              x, w_u, bias, act, residual, out)


# K22: a dense 3x3 stride-2 convolution of f32 tensors as an implicit GEMM on the f32 MFMA, with the K10 epilogue
# (csrc/conv3x3_strided.hip)

def pack_conv3x3_strided_weight(weight):
    """The [Cout, Cin, 3, 3] f32 convolution weight as mtr_conv3x3s2_bias_act takes it: a pure permutation to
    [Cin / 4, Cout, 3, 3, 4], element (c4, m, ky, kx, j) = w[m, 4 c4 + j, ky, kx], contiguous -- the 36 floats one
    output channel needs for a chunk of four input channels in one run, tap-major.  Plain torch; done once per weight."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.shape[1] % 4:
        raise ValueError(f'pack_conv3x3_strided_weight: expected [Cout, Cin, 3, 3] with Cin a multiple of 4, '
                         f'got {tuple(weight.shape)}')
    if weight.dtype != torch.float32:
        raise ValueError(f'pack_conv3x3_strided_weight: expected an f32 weight, got {weight.dtype}')
    M, K = weight.shape[:2]
    return weight.detach().reshape(M, K // 4, 4, 3, 3).permute(1, 0, 3, 4, 2).contiguous()


def _conv3x3_strided_weight_fits(w_packed, K):
    return w_packed.dim() == 5 and w_packed.dtype == torch.float32 and K % 4 == 0 \
        and tuple(w_packed.shape[2:]) == (3, 3, 4) and w_packed.shape[0] == K // 4 and w_packed.is_contiguous()


def conv3x3_strided_supported(x, w_packed):
    """Whether mtr_conv3x3s2_bias_act takes this input: CUDA f32 x [B, Cin, H, W], NCHW-contiguous and 16-byte
    aligned, w_packed [Cin / 4, Cout, 3, 3, 4] f32 contiguous (pack_conv3x3_strided_weight), Cin a multiple of 4, H and
    W even, W / 2 a multiple of 4 (its MTR_E_SHAPE / MTR_E_ALIGN rules, checked without a launch)."""
    return _dense3x3_supported(x, w_packed, _conv3x3_strided_weight_fits, 'mtr_conv3x3s2_lds_bytes')


def conv3x3_strided_bias_act(x, w_packed, bias, act, residual=None, out=None):
    """y = act(conv3x3(x, w, stride 2, padding 1) + bias) (+ residual) in one launch on the current stream, for f32:
    x [B, Cin, H, W] NCHW-contiguous, w_packed [Cin / 4, Cout, 3, 3, 4] (pack_conv3x3_strided_weight), bias [Cout] f32,
    residual [B, Cout, H / 2, W / 2] f32 or None.  One f32 fma chain per output element in a fixed order of (ci, ky,
    kx): the same bits on every call and graph replay, for any batch size."""
    return _dense3x3_bias_act('conv3x3_strided_bias_act', 'mtr_conv3x3s2_bias_act', 2, _conv3x3_strided_weight_fits,
                              'packed [{K} / 4, Cout, 3, 3, 4] and contiguous', x, w_packed, bias, act, residual, out)


# K20: a 1x1 stride-1 convolution of f32 tensors on the bf16 matrix cores, from operands split into three bf16 pieces
# (csrc/conv1x1_split.hip)

def _split_bf16x3(fn, w):
    """An f32 tensor as three bf16 pieces: p0 = bf16_rn(w), p1 = bf16_rn(w - p0), p2 = bf16_rn(w - p0 - p1), with
    p0 + p1 + p2 == w bit for bit, asserted in the name of the packer `fn`."""
    w0 = w.to(torch.bfloat16)
    r1 = w - w0.float()
    w1 = r1.to(torch.bfloat16)
    w2 = (r1 - w1.float()).to(torch.bfloat16)
    if not torch.equal(w0.float() + w1.float() + w2.float(), w):
        raise AssertionError(f'{fn}: the three bf16 pieces do not sum back to the weight '
                             '(non-finite or subnormal-range values)')
    return w0, w1, w2


def pack_conv1x1_split_weight(weight):
    """The [M, K] (or [M, K, 1, 1]) f32 weight as mtr_conv1x1_bias_act_split takes it: [3, M, Kp] bf16, Kp = K rounded
    up to 32 with a zero tail, w0 = bf16_rn(w), w1 = bf16_rn(w - w0), w2 = bf16_rn(w - w0 - w1).  The subtractions are
    exact in f32 and w0 + w1 + w2 == w bit for bit (asserted) for finite weights whose third piece does not underflow.
    Plain torch; done once per weight."""
    if weight.dim() not in (2, 4) or (weight.dim() == 4 and tuple(weight.shape[2:]) != (1, 1)):
        raise ValueError(f'pack_conv1x1_split_weight: expected [M, K] or [M, K, 1, 1], got {tuple(weight.shape)}')
    if weight.dtype != torch.float32:
        raise ValueError(f'pack_conv1x1_split_weight: expected an f32 weight, got {weight.dtype}')
    w = weight.detach().reshape(weight.shape[0], -1)
    M, K = w.shape
    w0, w1, w2 = _split_bf16x3('pack_conv1x1_split_weight', w)
    Kp = (K + 31) // 32 * 32
    out = torch.zeros(3, M, Kp, dtype=torch.bfloat16, device=w.device)
    out[0, :, :K], out[1, :, :K], out[2, :, :K] = w0, w1, w2
    return out


def conv1x1_split_supported(x, w_split):
    """Whether mtr_conv1x1_bias_act_split takes this input: CUDA f32 x [B, K, H, W], NCHW-contiguous and 16-byte
    aligned, w_split [3, M, Kp] bf16 contiguous (pack_conv1x1_split_weight), H*W and K multiples of 4 (its
    MTR_E_SHAPE / MTR_E_ALIGN rules, checked without a launch)."""
    if x.dim() != 4 or w_split.dim() != 3 or x.dtype != torch.float32 or w_split.dtype != torch.bfloat16 \
            or not x.is_cuda or not w_split.is_cuda or not x.is_contiguous() or not w_split.is_contiguous() \
            or x.data_ptr() % 16 or w_split.data_ptr() % 16:
        return False
    B, K, H, W = x.shape
    if w_split.shape[0] != 3 or w_split.shape[2] != (K + 31) // 32 * 32:
        return False
    return _lib.load().mtr_conv1x1_split_supported(B, w_split.shape[1], K, H * W) == 0


def conv1x1_bias_act_split(x, w_split, bias, act, gate=None, residual=None, in_bias=None, in_act=None, out=None):
    """conv1x1_bias_act for f32 tensors on the bf16 matrix cores (K20): y = act(conv1x1(v, w) + bias) (+ residual),
    v = in_act(x + in_bias) (x itself without in_bias) times gate[:, :, None, None], in one launch on the current
    stream.  x [B, K, H, W] f32 NCHW-contiguous, w_split [3, M, Kp] bf16 (pack_conv1x1_split_weight), bias [M],
    gate [B, K] f32 or None, residual [B, M, H, W] or None, in_bias [K] f32 or None.  The f32 product is summed from
    six bf16 products of the split operands in a fixed order: f32-grade against fp64 (K13's bound), the same bits on
    every call and graph replay, but not the bits of conv1x1_bias_act."""
    require_cuda(x, w_split, bias, gate, residual, in_bias)
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError('conv1x1_bias_act_split: x must be [B, K, H, W] f32, NCHW-contiguous')
    B, K, H, W = x.shape
    if w_split.dim() != 3 or w_split.shape[0] != 3 or w_split.dtype != torch.bfloat16 \
            or w_split.shape[2] != (K + 31) // 32 * 32 or not w_split.is_contiguous():
        raise ValueError(f'conv1x1_bias_act_split: the weight must be split [3, M, {(K + 31) // 32 * 32}] bf16 and '
                         f'contiguous for {K} input channels, got {tuple(w_split.shape)} {w_split.dtype}')
    M = w_split.shape[1]
    if bias.numel() != M:
        raise ValueError(f'conv1x1_bias_act_split: bias has {bias.numel()} elements, expected {M}')
    if gate is not None and (gate.dtype != torch.float32 or gate.numel() != B * K):
        raise ValueError('conv1x1_bias_act_split: gate must be [B, Cin] f32')
    if in_bias is None and in_act is not None:
        raise ValueError('conv1x1_bias_act_split: in_act needs in_bias')
    if in_bias is not None and (in_bias.dtype != torch.float32 or in_bias.numel() != K):
        raise ValueError('conv1x1_bias_act_split: in_bias must be [Cin] f32')
    out = _residual_and_out('conv1x1_bias_act_split', x, (B, M, H, W), residual, out)
    check(_lib.load().mtr_conv1x1_bias_act_split(
        _ptr(x), _ptr(w_split), _ptr(bias.contiguous().float()),
        None if in_bias is None else _ptr(in_bias.contiguous()), ACT_CODES[in_act],
        None if gate is None else _ptr(gate.contiguous()), None if residual is None else _ptr(residual),
        ACT_CODES[act], B, M, K, H * W, _ptr(out), current_stream_ptr(x.device)), 'mtr_conv1x1_bias_act_split')
    return out


# K21: a dense 3x3 stride-1 convolution of f32 tensors on the bf16 matrix cores, from operands split into three bf16
# pieces (csrc/conv3x3_split.hip)

CONV3X3_SPLIT_CHUNK = 16   # input channels per k step of K21: Cp of the packed weight is Cin rounded up to this


def pack_conv3x3_split_weight(weight):
    """The [Cout, Cin, 3, 3] f32 convolution weight as mtr_conv3x3_bias_act_split takes it: [3, Cout, 3, 3, Cp] bf16,
    contiguous, ci innermost, Cp = Cin rounded up to 16 with a zero tail; piece 0 = bf16_rn(w), piece 1 = bf16_rn(w -
    p0), piece 2 = bf16_rn(w - p0 - p1).  The subtractions are exact in f32 and p0 + p1 + p2 == w bit for bit
    (asserted) for finite weights whose third piece does not underflow.  Plain torch; done once per weight."""
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (3, 3) or weight.shape[1] % 8:
        raise ValueError(f'pack_conv3x3_split_weight: expected [Cout, Cin, 3, 3] with Cin a multiple of 8, '
                         f'got {tuple(weight.shape)}')
    if weight.dtype != torch.float32:
        raise ValueError(f'pack_conv3x3_split_weight: expected an f32 weight, got {weight.dtype}')
    w = weight.detach().permute(0, 2, 3, 1)   # [Cout, 3, 3, Cin]
    M, K = weight.shape[:2]
    w0, w1, w2 = _split_bf16x3('pack_conv3x3_split_weight', w)
    Kp = (K + CONV3X3_SPLIT_CHUNK - 1) // CONV3X3_SPLIT_CHUNK * CONV3X3_SPLIT_CHUNK
    out = torch.zeros(3, M, 3, 3, Kp, dtype=torch.bfloat16, device=w.device)
    out[0, ..., :K], out[1, ..., :K], out[2, ..., :K] = w0, w1, w2
    return out


def _conv3x3_split_weight_fits(w_split, K):
    return w_split.dim() == 5 and w_split.dtype == torch.bfloat16 and w_split.shape[0] == 3 \
        and tuple(w_split.shape[2:4]) == (3, 3) and K % 8 == 0 \
        and w_split.shape[4] == (K + CONV3X3_SPLIT_CHUNK - 1) // CONV3X3_SPLIT_CHUNK * CONV3X3_SPLIT_CHUNK \
        and w_split.is_contiguous()


def conv3x3_split_supported(x, w_split):
    """Whether mtr_conv3x3_bias_act_split takes this input: CUDA f32 x [B, Cin, H, W], NCHW-contiguous and 16-byte
    aligned, w_split [3, Cout, 3, 3, Cp] bf16 contiguous (pack_conv3x3_split_weight), Cin a multiple of 8, W a multiple
    of 4 (its MTR_E_SHAPE / MTR_E_ALIGN rules, checked without a launch)."""
    return _dense3x3_supported(x, w_split, _conv3x3_split_weight_fits, 'mtr_conv3x3_split_lds_bytes')


def conv3x3_bias_act_split(x, w_split, bias, act, residual=None, out=None):
    """y = act(conv3x3(x, w, stride 1, padding 1) + bias) (+ residual) in one launch on the current stream, for f32
    tensors on the bf16 matrix cores (K21): x [B, Cin, H, W] NCHW-contiguous, w_split [3, Cout, 3, 3, Cp] bf16
    (pack_conv3x3_split_weight), bias [Cout] f32, residual [B, Cout, H, W] f32 or None (it may be x).  The f32 product
    is summed from six bf16 products of the split operands in a fixed order: f32-grade against fp64, the same bits on
    every call and graph replay, for any batch size, but not the bits of the library's convolution."""
    return _dense3x3_bias_act('conv3x3_bias_act_split', 'mtr_conv3x3_bias_act_split', 1, _conv3x3_split_weight_fits,
                              'split [3, Cout, 3, 3, Cp] bf16 and contiguous for {K} input channels (a multiple of 8)',
                              x, w_split, bias, act, residual, out)
