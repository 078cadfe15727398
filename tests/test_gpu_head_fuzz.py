"""GPU: the fused head (mtr_head_fused_ws) and the stand-alone decode (mtr_softargmax_decode_opts) on cases DRAWN from
the domain they accept (tests/head_fuzz.py: four families of 24 seeded cases with a varied head config and five input
kinds; tests/test_head_fuzz_host.py holds the generators to the domain, to the places the draws must reach, and the
checker to rejecting subtly wrong answers).  One parametrized test per family and case.  Every case, through
metrabs_amd.kernels:

  * the DERIVED fp64 bound of head_fuzz.bound on every output element (no tolerance of this file's own), with the
    features / logits carved from NaN-filled buffers, coords2d and coords3d_rel inside sentinel bands and the workspace,
    where the shape has one, inside a sentinel-filled byte buffer: every output finite and written, all bands intact;
  * every kernel variant head_fuzz.variants finds for the case: the same bound; head32: the default's bits ("Every
    dispatch choice gives the same bits", include/metrabs_hip.h); head16: the default's bits within one layout;
  * the other layout: equal bits for f32 features, the bound for 16-bit ones;
  * crop 0 alone and crop B - 1 alone give the bits of their rows in the batch;
  * a second call into the same buffers gives the same bits; for two cases per family so does a captured graph's
    replay after the outputs were overwritten;
  * decode: the channels_last logits under nhwc_staging 0 .. 3: the bound; the bits of the walking kernel for 0 and 1,
    the bits of the staged kernel for 2 and 3, and the staged kernel on a crop alone.

Each test prints err / bound (max) and the kernel head_plan names; nothing is asserted about the ratio beyond <= 1."""
import pytest
import torch

import head_fuzz
from head_fuzz import GUARD, N_CASES, SENTINEL

pytestmark = pytest.mark.gpu
CASES = list(range(N_CASES))
GRAPH_CASES = (3, 14)
WS_FILL = 0xA5


def _workspace(lib, c, B, nhwc):
    """(buffer, workspace) -- the workspace of mtr_head_workspace_bytes at a 16-byte-aligned offset of a byte buffer
    filled with WS_FILL; (None, None) where the shape has none."""
    from metrabs_amd import _lib
    need = lib.mtr_head_workspace_bytes(_lib.dtype_code(c['dtype']), _lib.MTR_NHWC if nhwc else _lib.MTR_NCHW, B, c['C'],
                                        c['H'], c['W'], c['J'], c['D'])
    if not need:
        return None, None
    big = torch.full((need + 2 * GUARD,), WS_FILL, dtype=torch.uint8, device='cuda')
    ws = big[GUARD:GUARD + need]
    assert ws.data_ptr() % 16 == 0
    return big, ws


class _Launcher:
    """The case's inputs on the device in one layout (or a slice of the batch), and guarded launches on them."""

    def __init__(self, kernels, lib, c, inp, nhwc=None, crops=None):
        self.kernels, self.lib, self.c = kernels, lib, c
        self.dev = head_fuzz.on_device(c, inp, 'cuda', nhwc=nhwc, crops=crops)
        self.name = 'logits' if c['family'] == 'decode' else 'x'
        self.kept = self.dev[self.name].clone()
        self.B = self.kept.shape[0]
        self.case = dict(c, B=self.B)

    def buffers(self, workspace=True):
        c = self.c
        self.big2, c2d = head_fuzz.guarded_out((self.B, c['J'], 2), 'cuda')
        self.big3, c3d = head_fuzz.guarded_out((self.B, c['J'], 3), 'cuda')
        self.bigws, ws = (None, None)
        if c['family'] != 'decode' and workspace:
            self.bigws, ws = _workspace(self.lib, c, self.B, self.dev['nhwc'])
        self.out, self.ws = (c2d, c3d), ws
        return self.out

    def launch(self, **options):
        """The launch into self.out (self.ws), then the guard-band assertions."""
        use_ws = options.pop('workspace', True)
        kw = {}
        if self.c['family'] != 'decode':
            kw['workspace'] = (self.ws if self.ws is not None else None) if use_ws else False
        got = head_fuzz.run(self.kernels, self.case, self.dev, out=self.out, **kw, **options)
        assert got[0] is self.out[0] and got[1] is self.out[1]
        torch.cuda.synchronize()
        self.guards(options)
        return got

    def guards(self, what=''):
        assert head_fuzz.bands_intact(self.big2) and head_fuzz.bands_intact(self.big3), ('a write outside the outputs', what)
        if self.bigws is not None:
            assert bool((self.bigws[:GUARD] == WS_FILL).all()) and bool((self.bigws[-GUARD:] == WS_FILL).all()), \
                ('a write outside the workspace', what)
        assert head_fuzz.nan_bands_intact(self.dev['_big']) and torch.equal(self.dev[self.name], self.kept), \
            ('the input was written', what)
        for o in self.out:
            assert bool(torch.isfinite(o).all()), ('a read outside the input, or an overflow', what)
            assert not bool((o == SENTINEL).any()), ('an output element was not written', what)

    def fresh(self, **options):
        """A launch into new guarded buffers -> clones of the outputs."""
        self.buffers(workspace=options.get('workspace', True))
        return [o.clone() for o in self.launch(**options)]


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _replay(launcher):
    """A captured graph of the launch, replayed after the outputs were overwritten (the pattern of
    tests/test_gpu_se_gate2.py)."""
    with torch.inference_mode():
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            launcher.launch()
            st.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                head_fuzz.run(launcher.kernels, launcher.case, launcher.dev, out=launcher.out,
                              **({} if launcher.c['family'] == 'decode' else
                                 {'workspace': launcher.ws if launcher.ws is not None else None}))
        torch.cuda.current_stream().wait_stream(st)
        for o in launcher.out:
            o.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
    launcher.guards('graph replay')
    return [o.clone() for o in launcher.out]


def _case(family, i, hip_lib):
    from metrabs_amd import kernels
    c = head_fuzz.cases(family)[i]
    inp, _, _ = head_fuzz.truth(c)
    main = _Launcher(kernels, hip_lib, c, inp)
    main.buffers()
    first = [o.clone() for o in main.launch()]
    worst = head_fuzz.check(c, first, 'default')
    # a second call into the same buffers
    assert _same(main.launch(), first), 'a second call'
    if i in GRAPH_CASES:
        assert _same(_replay(main), first), 'graph replay'
    # crop 0 and crop B - 1 alone
    if c['B'] >= 2:
        for b in (0, c['B'] - 1):
            alone = _Launcher(kernels, hip_lib, c, inp, crops=slice(b, b + 1)).fresh()
            assert torch.equal(alone[0][0], first[0][b]) and torch.equal(alone[1][0], first[1][b]), f'crop {b} alone'
    return kernels, c, inp, main, first, worst


def _other_layout(kernels, hip_lib, c, inp, first, equal_bits):
    other = _Launcher(kernels, hip_lib, c, inp, nhwc=not c['nhwc'])
    got = other.fresh()
    r = head_fuzz.check(c, got, 'the other layout')
    if equal_bits:
        assert _same(got, first), 'the other layout'
    return other, got, r


def _heads(family, i, hip_lib):
    kernels, c, inp, main, first, worst = _case(family, i, hip_lib)
    label = lambda p: f"{p['kernel']} {p['tiles_per_workgroup']}x{p['column_blocks']}/{p['split_column_blocks']}"
    names = [f'{label(head_fuzz.plan(kernels, c))} = {worst:.3f}']
    for opts, p in head_fuzz.variants(kernels, c):
        got = main.fresh(**dict(opts))
        r = head_fuzz.check(c, got, opts)
        worst = max(worst, r)
        if family != 'head16rt':
            assert _same(got, first), (opts, p)
        names.append(f'{label(p)} = {r:.3f}')
    if c['C'] % 4 == 0:
        other, got, r = _other_layout(kernels, hip_lib, c, inp, first, equal_bits=family == 'head32')
        worst = max(worst, r)
        names.append(f'{label(head_fuzz.plan(kernels, c, nhwc=not c["nhwc"]))} (other layout) = {r:.3f}')
        if family == 'head16':      # the other layout's variants: its own default's bits
            for opts, p in head_fuzz.variants(kernels, c, nhwc=not c['nhwc']):
                alt = other.fresh(**dict(opts))
                r = head_fuzz.check(c, alt, opts)
                worst = max(worst, r)
                assert _same(alt, got), (opts, p)
                names.append(f'{label(p)} (other layout) = {r:.3f}')
    print(f'[head fuzz] {family} {head_fuzz.case_id(c)}: err / bound {worst:.3f}; {len(names)} launches: ' + '; '.join(names))


@pytest.mark.parametrize('i', CASES)
def test_head32(i, hip_lib):
    _heads('head32', i, hip_lib)


@pytest.mark.parametrize('i', CASES)
def test_head16(i, hip_lib):
    _heads('head16', i, hip_lib)


@pytest.mark.parametrize('i', CASES)
def test_head16rt(i, hip_lib):
    _heads('head16rt', i, hip_lib)


@pytest.mark.parametrize('i', CASES)
def test_decode(i, hip_lib):
    kernels, c, inp, main, first, worst = _case('decode', i, hip_lib)
    # the other layout: another kernel, the same bound
    other, got, r = _other_layout(kernels, hip_lib, c, inp, first, equal_bits=False)
    worst = max(worst, r)
    nhwc, walked = (main, first) if c['nhwc'] else (other, got)
    # The channels_last logits under nhwc_staging 0 .. 3.  Two kernels: the walking one (0 on these launches of fewer than
    # 256 crops, and 1) and the LDS-staged one (2, 3: one or two crops per workgroup) where the shape allows it -- the
    # walking one else.  Each pair has the same bits.  Across the pair the sums are the same only where the walking
    # kernel gives a channel ONE position group, which a small launch does not (tests/test_gpu_decode_recon.py compares
    # them on launches of 256 crops and more): here both are held to the bound, and whether the bits agree is reported.
    by_staging = {}
    for staging in (0, 1, 2, 3):
        by_staging[staging] = nhwc.fresh(nhwc_staging=staging)
        worst = max(worst, head_fuzz.check(c, by_staging[staging], f'nhwc_staging {staging}'))
    assert _same(by_staging[0], walked) and _same(by_staging[1], walked), 'nhwc_staging 0 / 1: the walking kernel'
    assert _same(by_staging[3], by_staging[2]), 'nhwc_staging 3: two crops per workgroup'
    # the staged kernel on crop 0 and on crop B - 1 alone
    if c['B'] >= 2:
        for b in (0, c['B'] - 1):
            alone = _Launcher(kernels, hip_lib, c, inp, nhwc=True, crops=slice(b, b + 1)).fresh(nhwc_staging=2)
            assert torch.equal(alone[0][0], by_staging[2][0][b]) and torch.equal(alone[1][0], by_staging[2][1][b]), \
                f'nhwc_staging 2: crop {b} alone'
    print(f'[head fuzz] decode {head_fuzz.case_id(c)}: err / bound {worst:.3f}; mtr_softargmax_decode_opts, staging 0 .. 3; '
          f'staged bits {"equal" if _same(by_staging[2], walked) else "differ from"} the walking kernel\'s')
