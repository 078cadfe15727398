"""CPU: the shape queries of K25h, K26h and K27h (mtr_expand_dw16_lds_bytes, mtr_expand_dw16_planes_lds_bytes,
mtr_expand_dw16_tiles_lds_bytes at stride 1 and 2) answer over a grid of shapes what the library answered BEFORE the
three kernels were put on one shared header (csrc/expand_dw16.h): every shape rule, tile choice, band height and LDS
size, pinned through the merge by tests/golden/expand_dw16_lds_bytes.json.

The fixture is recorded answers, not code.  To regenerate it on purpose, from a build of the commit whose answers are
to be pinned:

    python tests/test_expand_dw16_query_golden.py [path/to/libmetrabs_hip.so]
"""
import ctypes
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'expand_dw16_lds_bytes.json')
BS = (1, 8, 9)
CINS = (8, 16, 24, 40, 136)
CMIDS = (8, 32, 72, 200, 960)
SIDES = tuple(range(2, 37, 2)) + (48, 64, 96, 128, 132)   # H and W
QUERIES = (('k25h', 'mtr_expand_dw16_lds_bytes', ()), ('k26h', 'mtr_expand_dw16_planes_lds_bytes', ()),
           ('k27h_s1', 'mtr_expand_dw16_tiles_lds_bytes', (1,)), ('k27h_s2', 'mtr_expand_dw16_tiles_lds_bytes', (2,)))


def answers(lib):
    """{query: dict(planes=the distinct [H][W] tables of answers, each as runs [[bytes, count], ...] with W innermost;
    of=which table each (B, Cin, Cmid) has, B outermost and Cmid innermost)}."""
    out = {}
    for name, symbol, extra in QUERIES:
        q = getattr(lib, symbol)
        planes, of = [], []
        for B in BS:
            for Cin in CINS:
                for Cmid in CMIDS:
                    runs = []
                    for H in SIDES:
                        for W in SIDES:
                            v = int(q(B, Cin, Cmid, H, W, *extra))
                            if runs and runs[-1][0] == v:
                                runs[-1][1] += 1
                            else:
                                runs.append([v, 1])
                    if runs not in planes:
                        planes.append(runs)
                    of.append(planes.index(runs))
        out[name] = dict(planes=planes, of=of)
    return out


def test_the_shape_queries_answer_what_they_answered_before_the_merge():
    from metrabs_amd import _lib
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert golden['grid'] == dict(B=list(BS), Cin=list(CINS), Cmid=list(CMIDS), H=list(SIDES), W=list(SIDES))
    got = answers(_lib.load())
    for name, _, _ in QUERIES:
        want = golden['answers'][name]
        assert len(want['of']) == len(BS) * len(CINS) * len(CMIDS), name
        assert all(sum(c for _, c in runs) == len(SIDES) ** 2 for runs in want['planes']), name
        assert any(v > 0 for runs in want['planes'] for v, _ in runs), name   # (the grid reaches the kernel's domain)
        assert got[name] == want, name


if __name__ == '__main__':
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(here), 'metrabs_amd', 'csrc',
                                                              'libmetrabs_hip.so')
    lib = ctypes.CDLL(path)
    for _, symbol, extra in QUERIES:
        getattr(lib, symbol).restype = ctypes.c_size_t
        getattr(lib, symbol).argtypes = [ctypes.c_longlong] + [ctypes.c_int] * (4 + len(extra))
    doc = dict(grid=dict(B=list(BS), Cin=list(CINS), Cmid=list(CMIDS), H=list(SIDES), W=list(SIDES)),
               answers=answers(lib))
    with open(GOLDEN, 'w') as f:
        json.dump(doc, f, separators=(',', ':'))
        f.write('\n')
    print(GOLDEN, os.path.getsize(GOLDEN), 'bytes')
