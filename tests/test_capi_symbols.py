"""CPU: the C-ABI shared library loads and exports EVERY symbol include/metrabs_hip.h declares; the
ctypes table in metrabs_amd/_lib.py covers exactly that set; struct layouts match; argument checks
that need no GPU return the documented error codes (no compute calls here)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, 'include', 'metrabs_hip.h')


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = re.findall(r'^\s*(?:int|size_t|const char\*)\s+(mtr_\w+)\s*\(', text, flags=re.M)
    return sorted(set(names))


@pytest.fixture(scope='module')
def lib():
    from metrabs_amd import build, _lib
    build.build_library(verbose=False)  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_header_declares_expected_surface():
    names = declared_functions()
    assert len(names) >= 14 and 'mtr_softargmax_decode' in names and 'mtr_warp_crops' in names


def test_library_exports_every_declared_symbol(lib):
    from metrabs_amd import _lib
    for name in declared_functions():
        assert hasattr(lib, name), f'{name} is declared in the header but not exported'
    assert sorted(_lib.SIGNATURES) == declared_functions(), 'ctypes table out of sync with the header'


def test_struct_layouts_match_header():
    from metrabs_amd import _lib
    assert ctypes.sizeof(_lib.HeadParams) == 20 and ctypes.sizeof(_lib.ReconParams) == 36
    assert _lib.HeadParams.box_size_mm.offset == 16 and _lib.ReconParams.mix_3d_inside_fov.offset == 20
    text = open(HEADER).read()
    assert int(re.search(r'#define MTR_WARP_PARAM_FLOATS (\d+)', text).group(1)) == _lib.MTR_WARP_PARAM_FLOATS


def _header_without_comments():
    return re.sub(r'/\*.*?\*/', ' ', open(HEADER).read(), flags=re.S)


def _c_kind(decl):
    """One parameter (or return type) of a prototype -> 'ptr', 'int', 'long long', 'size_t', 'float' or 'double'."""
    decl = ' '.join(decl.split())
    if '*' in decl or re.search(r'\bmtr_stream_t\b', decl):
        return 'ptr'
    words = [w for w in re.findall(r'[A-Za-z_]\w*', decl) if w not in ('const', 'unsigned', 'signed')]
    for kind in ('long long', 'size_t', 'float', 'double', 'int'):
        if words[:len(kind.split())] == kind.split():
            return kind
    raise AssertionError(f'unknown parameter type in the header: {decl!r}')


def declared_prototypes():
    """name -> (return kind, [argument kinds]) of every function include/metrabs_hip.h declares."""
    protos = {}
    for m in re.finditer(r'^\s*(int|size_t|const char\s*\*)\s*(mtr_\w+)\s*\(([^;{]*?)\)\s*;',
                         _header_without_comments(), flags=re.M | re.S):
        ret, name, args = m.groups()
        args = args.strip()
        kinds = [] if args in ('', 'void') else [_c_kind(a) for a in args.split(',')]
        protos[name] = (_c_kind(ret), kinds)
    return protos


def _ctypes_kind(t):
    if t is int:   # (mtr_conv1x1_split_supported: the C int read into Python's int, see _lib.SIGNATURES)
        return 'int'
    scalars = {ctypes.c_int: 'int', ctypes.c_longlong: 'long long', ctypes.c_size_t: 'size_t',
               ctypes.c_float: 'float', ctypes.c_double: 'double'}
    assert len(scalars) == 5   # no two of them are one ctypes class on this platform
    if t in scalars:
        return scalars[t]
    if t in (ctypes.c_void_p, ctypes.c_char_p) or isinstance(t, type(ctypes.POINTER(ctypes.c_int))):
        return 'ptr'
    raise AssertionError(f'unknown ctypes type in _lib.SIGNATURES: {t!r}')


def test_the_prototype_parser_reads_what_it_is_given():
    protos = declared_prototypes()
    assert sorted(protos) == declared_functions()
    assert protos['mtr_version'] == ('int', []) and protos['mtr_strerror'] == ('ptr', ['int'])
    assert protos['mtr_head_packed_bytes'] == ('size_t', ['int'] * 4)
    assert protos['mtr_conv1x1_plan'] == ('int', ['int', 'int', 'int', 'long long', 'int', 'ptr'])
    assert _c_kind('const mtr_detector_geom* g') == 'ptr' and _c_kind('mtr_stream_t stream') == 'ptr'
    assert _c_kind('long long B') == 'long long' and _c_kind('size_t workspace_bytes') == 'size_t'
    assert _ctypes_kind(ctypes.POINTER(ctypes.c_int32)) == 'ptr' and _ctypes_kind(ctypes.c_longlong) == 'long long'


def test_ctypes_argument_lists_match_the_header():
    """Count and kind (pointer / stream, int, long long, size_t, float, double) of every argument, and the return
    type: a `long long B` bound as c_int in the middle of 17 arguments shifts nothing on x86-64 and reads garbage."""
    from metrabs_amd import _lib
    protos = declared_prototypes()
    assert sorted(protos) == sorted(_lib.SIGNATURES)
    for name, (restype, argtypes) in sorted(_lib.SIGNATURES.items()):
        ret, kinds = protos[name]
        assert _ctypes_kind(restype) == ret, (name, restype, ret)
        assert [_ctypes_kind(a) for a in argtypes] == kinds, (name, [_ctypes_kind(a) for a in argtypes], kinds)


STRUCTS = {'mtr_head_params': 'HeadParams', 'mtr_head_options': 'HeadOptions', 'mtr_head_plan_info': 'HeadPlanInfo',
           'mtr_recon_params': 'ReconParams', 'mtr_detector_geom': 'DetectorGeom', 'mtr_filter_params': 'FilterParams'}


def header_struct_fields():
    """struct name -> its field names in order, for every struct include/metrabs_hip.h defines."""
    structs = {}
    for m in re.finditer(r'typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;', _header_without_comments(), flags=re.S):
        assert m.group(1) == m.group(3)
        names = []
        for decl in m.group(2).split(';'):
            if decl.strip():
                first, *rest = decl.split(',')
                names += [first.split()[-1]] + [r.strip() for r in rest]
        structs[m.group(1)] = names
    return structs


def test_every_struct_layout_matches_the_header(tmp_path):
    """sizeof and every offsetof, as the host C compiler lays the header's six structs out, against the ctypes classes."""
    import shutil
    import subprocess
    from metrabs_amd import _lib
    fields = header_struct_fields()
    assert sorted(fields) == sorted(STRUCTS)
    cc = next((c for c in (os.environ.get('CC'), 'cc', 'gcc', 'clang') if c and shutil.which(c)), None)
    assert cc, 'no host C compiler'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "metrabs_hip.h"', 'int main(void) {']
    for s, names in sorted(fields.items()):
        lines.append(f'  printf("{s} sizeof %zu\\n", sizeof({s}));')
        for f in names:
            lines.append(f'  printf("{s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));')
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines) + '\n')
    subprocess.run([cc, '-std=c99', '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split('\n')
    seen = {s: [] for s in fields}
    for s, f, *nums in (l.split() for l in out if l):
        cls = getattr(_lib, STRUCTS[s])
        if f == 'sizeof':
            assert ctypes.sizeof(cls) == int(nums[0]), (s, ctypes.sizeof(cls), nums)
        else:
            d = getattr(cls, f)
            assert (d.offset, d.size) == (int(nums[0]), int(nums[1])), (s, f, d.offset, d.size, nums)
            seen[s].append(f)
    for s, names in fields.items():
        assert seen[s] == names == [n for n, _ in getattr(_lib, STRUCTS[s])._fields_], s


def test_version_strerror_and_host_side_argument_checks(lib):
    from metrabs_amd import _lib
    assert lib.mtr_version() == 100
    assert lib.mtr_strerror(0) == b'ok' and b'workspace' in lib.mtr_strerror(-5)
    hp = _lib.HeadParams(256, 32, 1, 0, 2200.0)
    # NULL pointers / bad shapes are rejected on the host before any launch
    assert lib.mtr_softargmax_decode(None, 0, 0, 1, 17, 8, 8, 8, ctypes.byref(hp), None, None, None) == -1
    assert lib.mtr_reconstruct_absolute(None, None, None, 1, 17, None, None, None, 0, None) == -1
    assert lib.mtr_warp_crops(None, None, None, 1, 8, 8, None, 1, 8, 1, 0, 0, None, None) == -1
    # f32 features: the row-tile blob = 40 stages x 10 tiles x 2 KiB + 160 rows x (bias f32 + label i32)
    assert lib.mtr_head_packed_bytes(1280, 17, 8, 0) == 40 * 10 * 2048 + 160 * 8
    # 72 depth bins (the metric string's shape): 17 atoms of 5 row tiles
    assert lib.mtr_head_packed_bytes(1280, 17, 72, 0) == 40 * 85 * 2048 + 85 * 16 * 8
    assert lib.mtr_head_packed_bytes(1280, 17, 81, 0) == 0  # > 80 depth bins: library GEMM + decode
    # f16 features: 3 joint groups x 64 rows of bias (f32) + 3 x 20 stages x 64 rows x 64 channels x 2 B
    # + the 16-bit row-tile section (C % 64 == 0): 20 stages x 10 tiles x 2 KiB + 160 rows x 8 B
    joint_groups = 3 * 64 * 4 + 3 * 20 * 64 * 64 * 2
    # + (round 5) the joint-group weights once more, fragment-major (whole 64-channel stages): 3 x 20 x 8 KiB
    assert lib.mtr_head_packed_bytes(1280, 17, 8, 1) == joint_groups + 20 * 10 * 2048 + 160 * 8 + 3 * 20 * 8192
    assert lib.mtr_head_packed_bytes(1283, 17, 8, 1) == 0   # C % 8 != 0: no 16-byte operands
    assert lib.mtr_head_packed_bytes(1288, 17, 8, 1) == 3 * 64 * 4 + 3 * 21 * 64 * 64 * 2  # C % 64 != 0: joint groups only
    # a joint's 73 rows exceed the 64-row group: the row-tile section alone (17 atoms of 5 tiles)
    assert lib.mtr_head_packed_bytes(1280, 17, 72, 2) == 20 * 85 * 2048 + 85 * 16 * 8
    assert lib.mtr_head_packed_bytes(1288, 17, 72, 2) == 0
    # the workspace of mtr_head_fused_ws: f32 maps of > 64 positions (column-block statistics), 16-bit
    # row-tile shapes (an NHWC copy of NCHW features + the statistics)
    assert lib.mtr_head_workspace_bytes(0, 0, 64, 1280, 8, 8, 17, 8) == 0
    assert lib.mtr_head_workspace_bytes(0, 0, 32, 1280, 12, 12, 17, 8) == 32 * 3 * 160 * 5 * 8
    assert lib.mtr_head_workspace_bytes(1, 0, 64, 1280, 8, 8, 17, 8) == 0
    assert lib.mtr_head_workspace_bytes(1, 0, 64, 1280, 8, 8, 17, 72) == 64 * 1280 * 64 * 2
    assert lib.mtr_head_workspace_bytes(1, 1, 64, 1280, 8, 8, 17, 72) == 0
    assert lib.mtr_reconstruct_workspace_bytes(64, 17) == (4 + 2 * 16) * 8


def test_product_never_imports_the_oracle():
    """The product path must not route through oracle/ (checked statically)."""
    pkg = os.path.join(ROOT, 'metrabs_amd')
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith('.py'):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r'^\s*(from|import)\s+oracle\b', src, flags=re.M), f


def test_missing_library_fails_loudly(tmp_path):
    from metrabs_amd import _lib
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _lib.load(str(tmp_path / 'nope.so'))


def test_every_entry_point_rejects_null_pointers_on_the_host(lib):
    """All pointer arguments NULL, integers 1, floats 1.0: every int-returning entry point answers
    MTR_E_NULL before it touches a device (no GPU here), none dereferences first."""
    from metrabs_amd import _lib
    checked = 0
    for name, (res, args) in sorted(_lib.SIGNATURES.items()):
        if res is not ctypes.c_int or name == 'mtr_version':
            continue
        vals = []
        for a in args:
            if a in (ctypes.c_int, ctypes.c_uint, ctypes.c_size_t, ctypes.c_longlong):
                vals.append(1)
            elif a in (ctypes.c_float, ctypes.c_double):
                vals.append(1.0)
            else:
                vals.append(None)  # data pointers, parameter structs, the stream
        assert getattr(lib, name)(*vals) == -1, name
        checked += 1
    assert checked >= 16
