"""Seeded fuzz of K8, the plausibility filter + pose NMS (mtr_filter_poses: csrc/pose_filter.hip), with every decision
PLACED a known, small distance from its threshold: a helper of tests/test_filter_fuzz_host.py (CPU) and
tests/test_gpu_filter_fuzz.py (GPU), no test module itself.

N_CASES calls from random.Random(SEED) over the table SCHEDULE (J, A, skeleton, order, var_correction, parameter set:
every value balanced over the set, nothing drawn and rejected).  A call has 1 .. 5 images with ragged pose counts
(COUNTS: 0 first, in the middle and last; 5 = one more than the 4 waves of the pose loop; up to 12).  Every pose
belongs to a CLASS; a class that needs a value solved for finds it by bisection on the fp64 yardstick of the f32
inputs (each placement is monotone in one scalar).  DELTA = 2^-12: a statistic "on side s" is its threshold times
(1 + s DELTA).

    plain           valid, far from everything
    bone1 s         one bone's ratio at rel_big, its difference far above abs_diff_mm (a 400 mm bone)
    bone2 s         ratio well above rel_big, the difference at abs_diff_mm (a 100 mm bone at 4x)
    bone3 s         ratio at rel_small, the difference far above (a 400 mm bone)
    bone4 s         ratio well below rel_small, the difference at abs_diff_mm (a 1.1 abs_diff_mm bone at 0.1 abs_diff_mm)
                    -- one bone critical, every other bone at ratio 1
    stdev s         exactly J / 4 joints clearly stable (<= 0.75 stdev_mm), one joint at stdev_mm on side s, the rest
                    clearly unstable (>= 1.25 stdev_mm), all measured after the scale-align: one global factor on the
                    perturbations places the critical joint.  s = -1: J / 4 + 1 stable, consistent; s = +1: J / 4, not
    box x|y s       the intersection area at box_fraction w h on side s, the box cut along x or y
    box_eq          the area EXACTLY box_fraction w h (integers): the strict '>' says no
    pair1 s         two valid poses at sim_threshold on side s: every joint moved by the same vector
    pair2 s         exactly k = J / 4 joints moved: the k LARGEST distances decide
    pair3 s         m joints moved past sim_scale_mm (2.2x) and k - m moved near: the ReLU decides.  m is the largest
                    count that leaves (k - m) / k >= 1.5 sim_threshold, at least 1: k - 1 where 1 / k allows it, and
                    1 of 4 at J = 17, 5 of 15 at J = 63 (with k - 1 far a pair of k >= 3 cannot reach 0.4 at all)
    chain o         A ~ B, B ~ C (0.6), A !~ C (0.2); the score orders o = 0, 1, 2 keep {A, C}, {B}, {C, A}
    A = 1           var_correction 1: 0 / 0, every stdev NaN, nothing valid; var_correction 0: everything stable

The poses of an image are shuffled, so invalid ones lie between valid ones (the compact nv x nv matrix differs from
n x n).  Skeletons: 'coco17' and 'chain' (J_model == J), 'coco_sub' / 'chain_sub' (J_model < J: the joints from J_model
up lie at 1e5 mm, every edge inside J_model), 'chain_past' (the same, and the table ALSO carries rows that reach past
J_model, which the kernel skips -- the only way a kernel that ignores J_model can be told apart), 'none', 'many'
(a chain listed forwards and backwards until it has more than 64 rows).  Pairs and chains are placed only where
J_model == J (a joint at 1e5 mm would multiply the similarity bound by 30).

YARDSTICK.  yardstick(case) is one fp64 evaluation from the f32 inputs as the kernel consumes them; it takes the
parameter set (the oracle hard-codes it) and indexes the joints (cpu_ref.joint2bone_mat is float32).  The mean pose is
carried twice: mean64, the fp64 mean, and mean32, the in-order float32 loop (s = s + x_a for a = 0 .. A - 1, then
s / A), which the kernel must reproduce BIT FOR BIT (__fadd_rn, __fdiv_rn).  The bones and the similarity are evaluated
in fp64 FROM mean32: a right kernel owns exactly those bits, so the only error left is its downstream rounding.

BOUNDS, u = 2^-24.
  mean pose    A - 1 additions in order and one division: |mean32 - mean64| <= A u mean_a |x_a| per element.
  similarity   from the f32 mean poses P_u, P_v.  One rounding each for: the square scale s (the kernel sums in f64
               and rounds once: e_s = 1 u relative; ANY f32 evaluation of 3J squares, their sum and the division:
               e_s = (3J + 2) u -- scale_u_f32(J)); msq = (s_u + s_v) / 2 (+1, the halving is exact); the quotient
               msq / s (+ e_s + 1); the root (halves what came in, + 2 for a root good to 1 ulp): f carries
               E_f = (e_s + 3) u.  The product f P: + 1; the rounded difference: + 1 on |f_u P_u| + |f_v P_v|; the
               norm (three squares, two additions, a root: 3 u d, d <= the L1 sum below).  So, per joint,
                   e_d(j) = (e_s + 8) u L1_j,    L1_j = sum_c |f_u P_u,j,c| + |f_v P_v,j,c|.
               The quotient d / scale (u q, and the ReLU forgets it past q = 2: <= 2 u), the subtraction (1 u), then
               the mean of k values in [0, 1] (the kernel: f64 and one rounding, 1 u; any f32 order: k u).  The mean
               of the k largest, the ReLU and 1 - d / scale are 1-Lipschitz in the maximum norm:
                   |sim - sim64| <= max_j e_d(j) / sim_scale + (3 + m) u,   m = 1 (kernel) or k (f32 oracle).
               The count is 4 for the kernel.
  not stored   the kernel evaluates them in f64 from f32 data and rounds to f32:
               bone: len 1 u, ratio = len / mean one more: 2 u ratio; diff = |len - mean|: u (len + diff);
               stdev: 2 u sd (one rounding, 1 u left for the f64 sums);
               box: the 2D mean is the in-order f32 loop too (the cases' 2D coordinates are multiples of 1/64 px
               below 2048, so A <= 65 of them add exactly in any order; the division rounds once): per axis
               e_i = u (2 (|hi| + |lo|) + i) for i = min(b + w, hi) - max(b, lo); area: e_ix iy + e_iy ix + u area;
               threshold box_fraction w h: 2 u.  'box_eq' is exact by construction (integers, a binary fraction).

MARGIN.  margin(case) = the smallest |statistic - threshold| / bound over EVERY comparison of the case (every bone
row of every pose, every joint's stdev, every box, every pair of valid poses); the host test holds it at >= 8.  The
bone, stdev and box classes reach it at DELTA = 2^-12; the pair classes use DELTA_PAIR (see there).

  * cases(); yardstick(case, params=None, variant=()); answer(case, y) -> what run() returns; margin(case);
  * check(case, ref, got) -> (failures, shares); wrong(kind, case) -> a subtly wrong answer (WRONG);
  * run(lib, case, device) -> the launch through ctypes, outputs inside guard bands, the caller's own
    NaN-filled workspace read back.
"""
import math
import random

import numpy as np

SEED = 80808
N_CASES = 24
U = 2.0 ** -24
DELTA = 2.0 ** -12
# the pair classes: the bound is 9 u L1 / sim_scale + 4 u with L1 ~ 1e4 mm (two people 2 m from the camera, |x| + |y| +
# |z| each), about 2e-5; sim_threshold 2^-12 is 1e-4: a margin of 5.  2^-11 is the smallest power of two that gives 8
DELTA_PAIR = 2.0 ** -11
GUARD = 64
F32, F64 = np.float32, np.float64

DEFAULTS = dict(rel_small=0.1, rel_big=3.0, abs_diff_mm=300.0, stdev_mm=200.0, box_fraction=0.5, sim_scale_mm=300.0,
                sim_threshold=0.4, max_output=150)
ALT = dict(rel_small=0.2, rel_big=2.5, abs_diff_mm=250.0, stdev_mm=150.0, box_fraction=0.375, sim_scale_mm=250.0,
           sim_threshold=0.5, max_output=3)

J_VALUES = (3, 4, 5, 7, 17, 40, 63, 64, 65, 122, 129)   # k = 0, k = 1; odd: the LDS rounding; 64 | 65; a third step
A_VALUES = (1, 2, 3, 8, 9, 65)
SKELETONS = ('coco17', 'chain', 'coco_sub', 'chain_sub', 'chain_past', 'none', 'many')
COCO17_EDGES = [(0, 1), (0, 2), (1, 3), (2, 4), (5, 6), (5, 7), (7, 9), (6, 8), (8, 10), (5, 11), (6, 12), (11, 12),
                (11, 13), (13, 15), (12, 14), (14, 16)]
_COCO17_XY = [(0, -700), (60, -760), (-60, -760), (160, -700), (-160, -700), (200, -450), (-200, -450), (300, -150),
              (-300, -150), (320, 150), (-320, 150), (130, 100), (-130, 100), (150, 550), (-150, 550), (160, 950),
              (-160, 950)]
# (J, A, skeleton, J_model, order_by_score, var_correction, alternative parameters)
SCHEDULE = (
    (17, 3, 'coco17', 17, 0, 0, 0), (3, 2, 'chain', 3, 1, 1, 0), (4, 8, 'chain', 4, 0, 1, 1), (5, 9, 'many', 5, 1, 0, 0),
    (7, 1, 'chain', 7, 0, 0, 1), (40, 2, 'coco_sub', 17, 1, 1, 0), (63, 3, 'chain', 63, 0, 0, 1), (64, 8, 'none', 64, 1, 1, 0),
    (65, 2, 'chain_past', 40, 0, 0, 1), (122, 3, 'chain', 122, 1, 1, 0), (129, 2, 'chain_sub', 122, 0, 0, 1),
    (17, 65, 'coco17', 17, 1, 0, 0), (3, 1, 'none', 3, 0, 1, 0), (4, 9, 'many', 4, 1, 0, 1), (5, 65, 'chain', 5, 0, 1, 0),
    (7, 3, 'chain_past', 5, 1, 0, 0), (40, 8, 'chain', 40, 0, 1, 1), (63, 9, 'many', 63, 1, 0, 0), (64, 2, 'chain', 64, 1, 1, 1),
    (65, 3, 'none', 65, 0, 1, 0), (122, 8, 'coco_sub', 17, 1, 0, 1), (129, 1, 'chain', 129, 0, 0, 0),
    (17, 9, 'coco17', 17, 1, 1, 1), (40, 65, 'chain_sub', 17, 0, 0, 1),
)
# pose counts per image; an empty image first (0), in the middle (1) and last (2); where A = 65 or J >= 122 a handful
COUNTS = ([0, 5, 3], [4, 0, 1], [2, 12, 0], [5, 1, 2, 3, 4], [7, 4], [3, 5], [12], [9, 0, 2], [6, 1], [3, 2], [4], [3, 3],
          [2, 0], [5, 8, 1, 0, 2], [4], [10, 3], [11, 5], [6, 0, 7], [1, 5, 4], [8, 2], [5], [3], [4, 9, 0, 3], [5])
# person slots (mm): the first ones lie nearest the axis and go to the pairs and chains (a smaller L1 in their bound)
_SLOTS = [(0, 0), (1300, 0), (-1300, 0), (0, 1300), (0, -1300), (1300, 1300), (-1300, 1300), (1300, -1300),
          (-1300, -1300), (2600, 0), (-2600, 0), (2600, 1300)]
# the round-robin of classes (size in poses, name, argument, side)
_ROBIN = ([(1, 'bone%d' % b, None, s) for b in (1, 2, 3, 4) for s in (1, -1)] + [(1, 'plain', None, 0)] +
          [(2, 'pair%d' % p, None, s) for p in (1, 2, 3) for s in (1, -1)] + [(1, 'stdev', None, 1), (1, 'stdev', None, -1)] +
          [(1, 'box', ax, s) for ax in (0, 1) for s in (1, -1)] + [(3, 'chain', o, 0) for o in (0, 1, 2)] +
          [(1, 'box_eq', None, 0), (1, 'plain', None, 0)])


def params_f32(p):
    """The thresholds as the kernel holds them: float32 values (as Python floats)."""
    return {k: (int(v) if k == 'max_output' else float(F32(v))) for k, v in p.items()}


def mean32(x):
    """torch.mean over the augmentation axis as the kernel does it: the float32 sum in order, one division."""
    s = np.zeros(x.shape[:1] + x.shape[2:], F32)
    for a in range(x.shape[1]):
        s = (s + x[:, a]).astype(F32)
    return (s / F32(x.shape[1])).astype(F32)


# ------------------------------------------------------------------------------------------------ the statistics, fp64

def bone_stats(M, edges, mean_bones):
    """M [P, J, 3] f64 -> (length, ratio, difference), each [P, n_bones]."""
    if len(edges) == 0:
        z = np.zeros((len(M), 0))
        return z, z, z
    e = np.asarray(edges)
    length = np.linalg.norm(M[:, e[:, 0]] - M[:, e[:, 1]], axis=-1)
    mb = np.asarray(mean_bones, F64)
    return length, length / mb, np.abs(length - mb)


def joint_stdev(p3, var_correction, align=True):
    """p3 [P, A, J, 3] f32 -> the per-joint standard deviation over A after the scale-align, [P, J] (NaN at A - ddof = 0)."""
    X = p3.astype(F64)
    A = X.shape[1]
    if align:
        sq = np.mean(np.square(X), axis=(2, 3), keepdims=True)
        X = X * np.sqrt(np.mean(sq, axis=1, keepdims=True) / sq)
    d = X - X.mean(axis=1, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        var = np.square(d).sum(axis=1) / F64(A - var_correction)
        return np.sqrt(var.sum(axis=-1))


def box_stats(m2, boxes):
    """m2 [P, J, 2] f64 (the mean 2D pose), boxes [P, 5] -> dict of per-pose lo, hi of the intersection, ix, iy, area and
    the full box area w h."""
    b = boxes.astype(F64)
    hi = np.minimum(b[:, :2] + b[:, 2:4], m2.max(axis=1))
    lo = np.maximum(b[:, :2], m2.min(axis=1))
    inter = np.maximum(hi - lo, 0.0)
    return dict(lo=lo, hi=hi, inter=inter, area=inter[:, 0] * inter[:, 1], box_area=b[:, 2] * b[:, 3])


def similarity(P, scale, top='largest', k=None, relu=True):
    """P [n, J, 3] f64 -> the [n, n] similarity matrix (NaN at k = 0) and the scaled poses' L1 sums [n, n, J]."""
    n, J = P.shape[:2]
    k = J // 4 if k is None else k
    s = np.mean(np.square(P), axis=(1, 2))
    msq = (s[:, None] + s[None, :]) / 2
    fu, fv = np.sqrt(msq / s[:, None]), np.sqrt(msq / s[None, :])
    Pu, Pv = fu[:, :, None, None] * P[:, None], fv[:, :, None, None] * P[None, :]
    d = np.linalg.norm(Pu - Pv, axis=-1)
    l1 = np.abs(Pu).sum(-1) + np.abs(Pv).sum(-1)
    if top == 'all':
        k = J
    if k == 0:
        return np.full((n, n), np.nan), l1
    d = np.sort(d, axis=-1)
    best = d[..., :k] if top == 'smallest' else d[..., J - k:]
    t = 1 - best / scale
    return np.mean(np.maximum(t, 0) if relu else t, axis=-1), l1


SCALE_U_KERNEL = 1


def scale_u_f32(J):
    return 3 * J + 2


def sim_bound(l1, scale, scale_u=SCALE_U_KERNEL, mean_u=1):
    """The bound on every entry of the similarity matrix (module docstring)."""
    return (scale_u + 8) * U * l1.max(axis=-1) / scale + (3 + mean_u) * U


def greedy_nms(sim, scores, thr, order_by_score, max_output, greedy=True, by_index=False):
    """Indices (into the valid list) that survive, in the output order."""
    n = len(scores)
    rank = list(range(n)) if by_index else sorted(range(n), key=lambda i: (-scores[i], i))
    state, kept = [0] * n, []
    for r, u in enumerate(rank):
        if state[u] == -1 and greedy:
            continue
        if state[u] == 0:
            if order_by_score and len(kept) >= max_output:
                continue
            kept.append(u)
        for v in rank[r + 1:]:
            if state[v] == 0 and sim[u, v] > thr:
                state[v] = -1
    return kept if order_by_score else sorted(kept)


WRONG = ('smallest_k', 'all_j', 'ceil_k', 'no_relu', 'no_scale_align', 'var_correction_flipped', 'count_ge', 'bone_or',
         'rel_small_ignored', 'j_model_ignored', 'box_ge', 'default_params', 'non_greedy', 'index_order', 'n_by_n')


def yardstick(case, params=None, variant=()):
    """One fp64 evaluation of the whole call (module docstring).  `variant`: names of WRONG, for wrong()."""
    v = set(variant)
    prm = params_f32(DEFAULTS if 'default_params' in v else (params or case['params']))
    p3, p2, boxes = case['poses3d'], case['poses2d'], case['boxes']
    P, A, J = p3.shape[:3]
    m32, m64 = mean32(p3), p3.astype(F64).mean(axis=1)
    M = m32.astype(F64)
    edges, mb = case['edges'], case['mean_bones']
    Jm = J if 'j_model_ignored' in v else case['J_model']
    active = np.array([j1 < Jm and j2 < Jm for j1, j2 in edges], bool)
    length, ratio, diff = bone_stats(M, edges, mb)
    out_of_range = ratio > prm['rel_big']
    if 'rel_small_ignored' not in v:
        out_of_range = out_of_range | (ratio < prm['rel_small'])
    off = diff > prm['abs_diff_mm']
    flagged = (out_of_range | off) if 'bone_or' in v else (out_of_range & off)
    plausible = ~np.any(flagged & active, axis=1) if len(edges) else np.ones(P, bool)
    varc = case['var_correction'] ^ (1 if 'var_correction_flipped' in v else 0)
    sd = joint_stdev(p3, varc, align='no_scale_align' not in v)
    with np.errstate(invalid='ignore'):
        n_stable = (sd < prm['stdev_mm']).sum(axis=1)
    consistent = (n_stable >= J // 4) if 'count_ge' in v else (n_stable > J // 4)
    bs = box_stats(mean32(p2).astype(F64), boxes)
    bthr = prm['box_fraction'] * bs['box_area']
    in_box = (bs['area'] >= bthr) if 'box_ge' in v else (bs['area'] > bthr)
    valid = plausible & consistent & in_box
    k = (J + 3) // 4 if 'ceil_k' in v else J // 4
    top = 'smallest' if 'smallest_k' in v else 'all' if 'all_j' in v else 'largest'
    sims, l1s, lists, kept = [], [], [], {0: [], 1: []}
    for lo, hi in zip(case['row_start'][:-1], case['row_start'][1:]):
        idx = [q for q in range(lo, hi) if valid[q]]
        sim, l1 = similarity(M[idx], prm['sim_scale_mm'], top=top, k=k, relu='no_relu' not in v) if idx \
            else (np.zeros((0, 0)), np.zeros((0, 0, J)))
        sims.append(sim)
        l1s.append(l1)
        lists.append(idx)
        for order in (0, 1):
            with np.errstate(invalid='ignore'):
                keep = greedy_nms(sim, [float(boxes[q, 4]) for q in idx], prm['sim_threshold'], order, prm['max_output'],
                                  greedy='non_greedy' not in v, by_index='index_order' in v)
            kept[order].append([idx[u] for u in keep])
    return dict(params=prm, mean32=m32, mean64=m64, length=length, ratio=ratio, diff=diff, active=active, sd=sd,
                n_stable=n_stable, box=bs, box_thr=bthr, plausible=plausible, consistent=consistent, in_box=in_box,
                valid=valid, valid_lists=lists, sim=sims, l1=l1s, kept=kept, n_by_n='n_by_n' in v)


def answer(case, y, order=None):
    """What run() returns, from a yardstick evaluation: the outputs and the workspace as the kernel leaves them."""
    order = case['order_by_score'] if order is None else order
    P = len(y['valid'])
    keep_idx, keep_count, sim = np.full(P, -1, np.int32), [], []
    for i, (lo, hi) in enumerate(zip(case['row_start'][:-1], case['row_start'][1:])):
        kept = y['kept'][order][i]
        keep_idx[lo:lo + len(kept)] = kept
        keep_count.append(len(kept))
        n, idx = hi - lo, y['valid_lists'][i]
        flat = np.full(n * n, np.nan, F32)
        for a, qa in enumerate(idx):
            for b, qb in enumerate(idx):
                flat[(qa - lo) * n + (qb - lo) if y['n_by_n'] else a * len(idx) + b] = y['sim'][i][a, b]
        sim.append(flat)
    return dict(valid=y['valid'].astype(np.uint8), keep_idx=keep_idx, keep_count=np.array(keep_count, np.int32),
                mean=y['mean32'].copy(), sim=sim, bands=True)


def wrong(kind, case):
    """A subtly wrong answer: the yardstick with one rule of WRONG changed."""
    assert kind in WRONG
    return answer(case, yardstick(case, variant=(kind,)))


def mean_bound(case):
    return case['poses3d'].shape[1] * U * np.abs(case['poses3d'].astype(F64)).mean(axis=1)


def check(case, ref, got):
    """-> (failures, shares): `got` (run() or answer()) against the yardstick `ref`.  failures: a list of strings,
    empty for a right answer; shares: the largest used share of the mean-pose bound and of the similarity bound."""
    fails, shares = [], dict(mean=0.0, sim=0.0)
    want = answer(case, ref)
    if not got['bands']:
        fails.append('a guard band was written')
    if got['mean'].tobytes() != ref['mean32'].tobytes():
        fails.append('mean pose: not the bits of the in-order float32 loop')
    err = np.abs(got['mean'].astype(F64) - ref['mean64'])
    mb = mean_bound(case)
    if not np.all(err <= mb):
        fails.append('mean pose: outside the fp64 bound')
    shares['mean'] = float(np.max(err / np.maximum(mb, 1e-300))) if err.size else 0.0
    for i, flat in enumerate(got['sim']):
        nv = len(ref['valid_lists'][i])
        block = flat[:nv * nv].reshape(nv, nv).astype(F64)
        want_s = ref['sim'][i]
        if not np.all(np.isnan(flat[nv * nv:])):
            fails.append(f'image {i}: workspace past the nv x nv block was written')
        if block.tobytes() != block.T.copy().tobytes():
            fails.append(f'image {i}: similarity not symmetric bit for bit')
        if nv == 0:
            continue
        if np.isnan(want_s).all():      # k = 0
            if not np.isnan(block).all():
                fails.append(f'image {i}: similarity not NaN at k = 0')
            continue
        bound = sim_bound(ref['l1'][i], ref['params']['sim_scale_mm'])
        e = np.abs(block - want_s)
        if not np.all(e <= bound):      # (a NaN fails too)
            fails.append(f'image {i}: similarity outside the bound, {float(np.nanmax(e / bound)):.3g} bounds')
        else:
            shares['sim'] = max(shares['sim'], float(np.max(e / bound)))
    for name in ('valid', 'keep_idx', 'keep_count'):
        if got[name].tolist() != want[name].tolist():
            fails.append(f'{name}: {got[name].tolist()} != {want[name].tolist()}')
    return fails, shares


def margin(case, y=None):
    """The smallest |statistic - threshold| / bound over every comparison of the case (module docstring)."""
    y = y or yardstick(case)
    prm, worst = y['params'], math.inf

    def take(stat, thr, bound):
        nonlocal worst
        stat, bound = np.asarray(stat, F64), np.asarray(bound, F64)
        ok = ~np.isnan(stat)
        if ok.any():
            worst = min(worst, float(np.min(np.abs(stat - thr)[ok] / np.maximum(bound[ok], 1e-300))))

    act = y['active']
    if act.any():
        ratio, diff, length = y['ratio'][:, act], y['diff'][:, act], y['length'][:, act]
        take(ratio, prm['rel_big'], 2 * U * ratio)
        take(ratio, prm['rel_small'], 2 * U * ratio)
        take(diff, prm['abs_diff_mm'], U * (length + diff))
    take(y['sd'], prm['stdev_mm'], 2 * U * y['sd'])
    bs = y['box']
    e_i = U * (2 * (np.abs(bs['hi']) + np.abs(bs['lo'])) + bs['inter'])
    e_area = e_i[:, 0] * bs['inter'][:, 1] + e_i[:, 1] * bs['inter'][:, 0] + U * bs['area'] + 2 * U * y['box_thr']
    exact = np.array([c[0] == 'box_eq' for c in case['classes']])
    assert np.all(bs['area'][exact] == y['box_thr'][exact])
    take(bs['area'][~exact], y['box_thr'][~exact], e_area[~exact])
    for sim, l1 in zip(y['sim'], y['l1']):
        if len(sim) > 1:
            off = ~np.eye(len(sim), dtype=bool)
            take(sim[off], prm['sim_threshold'], sim_bound(l1, prm['sim_scale_mm'])[off])
    return worst


# ------------------------------------------------------------------------------------------------ the generator

def _bisect(stat, lo, hi, target, side, thr):
    """The scalar t in [lo, hi] at which the monotone stat(t) sits at `target`, on side `side` of `thr`."""
    increasing = stat(hi) > stat(lo)
    assert (stat(lo) - target) * (stat(hi) - target) < 0, (stat(lo), stat(hi), target)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if (stat(mid) < target) == increasing:
            lo = mid
        else:
            hi = mid
    t = min((lo, hi), key=lambda x: abs(stat(x) - target))
    got = stat(t)
    assert abs(got / target - 1) < 2.0 ** -15 and (got - thr) * side > 0, (got, target, thr)
    return t


def _skeleton(kind, J, Jm, rng):
    """-> edges (list of pairs), the template T [J, 3] f64 (before the special bones), cut candidates: (the joints that
    move together, joint pair) for every bone that can be made critical without touching another."""
    T = np.zeros((J, 3))
    if kind in ('coco17', 'coco_sub'):
        T[:17, :2] = np.array(_COCO17_XY, F64)
        T[:17, 2] = [rng.uniform(-30, 30) for _ in range(17)]
        edges = list(COCO17_EDGES)
        cuts = [([3], (1, 3)), ([4], (2, 4)), ([9], (7, 9)), ([10], (8, 10))]
    else:
        for j in range(1, Jm):      # bones of 350 .. 500 mm in the x-y plane, turning by 2.4 rad: the cloud stays compact
            L, th = rng.uniform(350, 500), 2.4 * j
            T[j] = T[j - 1] + (L * math.cos(th), L * math.sin(th), rng.uniform(-30, 30))
        chain = [(j, j + 1) for j in range(Jm - 1)]
        edges = [] if kind == 'none' else list(chain)
        if kind == 'many':
            while len(edges) <= 64:
                edges += [(b, a) for a, b in chain] + chain
        if kind == 'chain_past':    # rows that reach past J_model: skipped by the kernel
            edges += [(j, j + 1) for j in range(Jm - 1, J - 1)]
        cuts = [] if kind == 'none' else [(list(range(c, Jm)), (c - 1, c)) for c in range(1, min(Jm, 5))]
    for j in range(Jm, J):          # wild joints
        T[j] = (1e5 * (1 if j % 2 else -1), 1e5 * (1 if j % 3 else -1), 1e5 + 10.0 * j)
    T[:Jm] -= T[:Jm].mean(axis=0)
    return edges, T, cuts


def _special_length(bone, prm):
    return {1: 400.0, 2: 100.0, 3: 400.0, 4: 1.1 * prm['abs_diff_mm']}[bone]


def _plan(i, J, Jm, skeleton, A, counts, n_cuts):
    """The classes of case i: per image a list of groups (name, argument, side), in slot order."""
    k = J // 4
    pointer, bones, images = (i * 7) % len(_ROBIN), [], []

    def fits(size, name, room):
        if size > room:
            return False
        if name.startswith('bone'):
            b = int(name[4])
            return b in bones or len(bones) < min(2, n_cuts)
        if name == 'stdev':
            return A >= 2
        if name in ('pair1', 'pair2', 'chain'):
            return Jm == J and k >= 1
        if name == 'pair3':
            return Jm == J and k >= 2
        return True

    for n in counts:
        groups, room = [], n
        while room:
            while not fits(_ROBIN[pointer][0], _ROBIN[pointer][1], room):
                pointer = (pointer + 1) % len(_ROBIN)
            size, name, arg, side = _ROBIN[pointer]
            pointer = (pointer + 1) % len(_ROBIN)
            if name.startswith('bone') and int(name[4]) not in bones:
                bones.append(int(name[4]))
            groups.append((size, name, arg, side))
            room -= size
        groups.sort(key=lambda g: -g[0])    # pairs and chains take the slots nearest the axis
        images.append(groups)
    return images, bones


def _movable(T, edges, Jm, prm, special_joints, vmax):
    """Joints that can move by up to vmax along z with every incident bone staying plausible by a wide margin."""
    ok = []
    for j in range(Jm):
        good = j not in special_joints
        for a, b in edges:
            if j in (a, b) and a < Jm and b < Jm:
                L = float(np.linalg.norm(T[a] - T[b]))
                good = good and math.hypot(L, vmax) / L < 0.9 * prm['rel_big']
        if good:
            ok.append(j)
    return ok


def build_case(i):
    J, A, skeleton, Jm, order, varc, alt = SCHEDULE[i]
    rng = random.Random(SEED * 1000 + i)
    params = dict(ALT if alt else DEFAULTS)
    prm = params_f32(params)
    counts = list(COUNTS[i])
    edges, T, cuts = _skeleton(skeleton, J, Jm, rng)
    plan, bones = _plan(i, J, Jm, skeleton, A, counts, len(cuts))
    special = {}                         # bone class -> (moving joints, (j1, j2), unit direction)
    for b, (moving, (j1, j2)) in zip(bones, cuts):
        d = T[j2] - T[j1]
        d /= np.linalg.norm(d)
        T[moving] += (T[j1] + d * _special_length(b, prm) - T[j2])
        special[b] = (moving, (j1, j2), d)
    mean_bones = np.array([np.linalg.norm(T[a] - T[b]) if a < Jm and b < Jm else 300.0 for a, b in edges], F32)
    special_joints = {j for _, (j1, j2), _ in special.values() for j in (j1, j2)}
    scale, thr_sim = prm['sim_scale_mm'], prm['sim_threshold']
    movable = _movable(T, edges, Jm, prm, special_joints, 2.2 * scale)
    k = J // 4
    w = [math.sqrt(2) * math.cos(2 * math.pi * a / A + math.pi / 4) for a in range(A)] if A > 1 else [0.0]
    ez = np.array([0.0, 0.0, 1.0])

    def aug_noise(base, amp):
        """[A, J, 3]: amp[j] * w[a] along a direction perpendicular to the joint (the square scale barely moves)."""
        d = np.cross(base, ez)
        d /= np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-9)
        sign = np.where(np.arange(J) % 2, -1.0, 1.0)
        return np.asarray(w)[:, None, None] * (amp * sign)[None, :, None] * d[None]

    def as_input(base, amp):
        return (base[None] + aug_noise(base, np.broadcast_to(np.asarray(amp, F64), (J,)))).astype(F32)   # [A, J, 3]

    def pose2d(lo, size, integers=False):
        """[A, J, 2] on the 1/64 px grid: joints 0 and 1 at the corners of [lo, lo + size], the rest inside."""
        q = np.array([[rng.uniform(0.05, 0.95), rng.uniform(0.05, 0.95)] for _ in range(J)])
        q[0], q[1] = (0, 0), (1, 1)
        if J > 2:
            q[2] = (0.5, 0.5)
        base = np.asarray(lo, F64) + q * np.asarray(size, F64)
        jit = np.array([[[rng.randrange(-64, 65) / 64.0, rng.randrange(-64, 65) / 64.0] for _ in range(J)] for _ in range(A)])
        jit[:, :2] = 0
        if integers:
            return np.broadcast_to(np.round(base), (A, J, 2)).astype(F32)
        return (np.round((base[None] + jit) * 64) / 64).astype(F32)

    p3, p2, bx, classes, row_start, scores_all = [], [], [], [], [0], []
    small = 0.015 * prm['stdev_mm']
    for groups in plan:
        poses, slot = [], 0
        for size, name, arg, side in groups:
            sx, sy = _SLOTS[slot]
            offset = np.array([sx, sy, 2000.0 + 60.0 * slot])
            slot += 1
            tangent = np.array([-offset[2], 0.0, offset[0]]) / math.hypot(offset[2], offset[0])   # the scale-align absorbs a radial move
            base = T + offset
            base[Jm:] = T[Jm:]
            lo2, size2 = (300.0 + 90 * slot, 200.0 + 40 * slot), (rng.randrange(120, 260), rng.randrange(200, 420))
            members = []                 # (pose3d [A, J, 3], class)
            if name.startswith('bone'):
                b = int(name[4])
                moving, (j1, j2), d = special[b]
                row = [(j1, j2)]
                L0 = _special_length(b, prm)

                def inp(t, base=base, moving=moving, d=d):
                    x = base.copy()
                    x[moving] += d * t
                    return as_input(x, small)

                def stat(t, which, inp=inp, row=row):
                    s = bone_stats(mean32(inp(t)[None]).astype(F64), row, [mean_bones[edges.index(row[0])]])
                    return float(s[which][0, 0])
                mbv = float(mean_bones[edges.index((j1, j2))])
                if b == 1:
                    t = _bisect(lambda t: stat(t, 1), (prm['rel_big'] - 1.2) * L0, (prm['rel_big'] - 0.8) * L0,
                                prm['rel_big'] * (1 + side * DELTA), side, prm['rel_big'])
                elif b == 3:
                    t = _bisect(lambda t: stat(t, 1), -0.95 * L0, -0.7 * L0, prm['rel_small'] * (1 + side * DELTA), side,
                                prm['rel_small'])
                else:
                    sgn = 1 if b == 2 else -1
                    t = _bisect(lambda t: stat(t, 2), sgn * 0.9 * prm['abs_diff_mm'], sgn * min(1.1 * prm['abs_diff_mm'], 0.999 * mbv if b == 4 else 1e9),
                                prm['abs_diff_mm'] * (1 + side * DELTA), side, prm['abs_diff_mm'])
                members.append((inp(t), (name, side)))
            elif name == 'stdev':
                cf = math.sqrt(A / (A - varc))
                joints = list(range(J))
                rng.shuffle(joints)
                amp = np.full(J, 2.2 * prm['stdev_mm'] / cf)
                amp[joints[:k]] = 0.3 * prm['stdev_mm'] / cf
                crit = joints[k]
                amp[crit] = prm['stdev_mm'] / cf

                def stat(g, base=base, amp=amp, crit=crit):
                    return float(joint_stdev(as_input(base, g * amp)[None], varc)[0, crit])
                g = _bisect(stat, 0.8, 1.25, prm['stdev_mm'] * (1 + side * DELTA), side, prm['stdev_mm'])
                x = as_input(base, g * amp)
                sd = joint_stdev(x[None], varc)[0]
                rest = np.delete(sd, crit) / prm['stdev_mm']
                assert (rest <= 0.75).sum() == k and (rest >= 1.25).sum() == J - 1 - k, rest
                members.append((x, (name, side, crit)))
            elif name.startswith('pair'):
                kind = int(name[4])
                xu = as_input(base, small)
                mu = mean32(xu[None]).astype(F64)
                if kind == 1:
                    near, far = list(range(J)), []
                    direction = tangent
                else:
                    m_far = 0
                    if kind == 3:
                        m_far = max(m for m in range(1, k) if m == 1 or (k - m) / k >= 1.5 * thr_sim)
                        assert (k - m_far) / k > 1.2 * thr_sim
                    assert len(movable) >= k, (J, skeleton, movable)
                    chosen = movable[-k:]
                    far, near = chosen[:m_far], chosen[m_far:]
                    direction = ez

                def inp(t, base=base, near=near, far=far, direction=direction):
                    x = base.copy()
                    x[near] += direction * t
                    x[far] += direction * 2.2 * scale
                    return as_input(x, 0.8 * small)

                def stat(t, inp=inp, mu=mu):
                    mv = mean32(inp(t)[None]).astype(F64)
                    return float(similarity(np.concatenate([mu, mv]), scale)[0][0, 1])
                t = _bisect(stat, 0.0, scale, thr_sim * (1 + side * DELTA_PAIR), side, thr_sim)
                members += [(xu, (name, side, 'u')), (inp(t), (name, side, 'v'))]
            elif name == 'chain':
                step = tangent * 0.67 * scale * (1 - thr_sim)
                members += [(as_input(base + s * step, small), (name, arg, 'ABC'[s + 1])) for s in (-1, 0, 1)]
            else:
                members.append((as_input(base, small), (name, arg, side) if name == 'box' else (name,)))
            for x, cls in members:
                if cls[0] == 'box_eq':
                    lo2 = (float(round(lo2[0])), float(round(lo2[1])))
                    y2 = pose2d(lo2, (256, 128), integers=True)
                    ix = prm['box_fraction'] * 256
                    box = [lo2[0] + 256 - ix, lo2[1], 256.0, 128.0]
                else:
                    y2 = pose2d(lo2, size2)
                    m2 = mean32(y2[None]).astype(F64)[0]
                    lo, hi = m2.min(axis=0), m2.max(axis=0)
                    box = [lo[0] - 8, lo[1] - 8, hi[0] - lo[0] + 16, hi[1] - lo[1] + 16]
                    if cls[0] == 'box':
                        ax, s = cls[1], cls[2]
                        box[2 + ax] = hi[ax] - lo[ax]

                        def stat(t, box=box, ax=ax, lo=lo, m2=m2):
                            bb = list(box)
                            bb[ax] = lo[ax] + t
                            bb = np.array([bb + [0.0]], F32)
                            r = box_stats(m2[None], bb)
                            return float(r['area'][0] / (prm['box_fraction'] * r['box_area'][0]))
                        t = _bisect(stat, 0.0, 0.9 * (hi[ax] - lo[ax]), 1 + s * DELTA, s, 1.0)
                        box[ax] = lo[ax] + t
                poses.append((x, y2, box, cls))
        order_idx = list(range(len(poses)))
        rng.shuffle(order_idx)
        ranks = list(range(len(poses)))
        rng.shuffle(ranks)
        score = {q: 0.3 + 0.6 * (r + 1) / (len(poses) + 1) for q, r in zip(range(len(poses)), ranks)}
        for q, (_, _, _, cls) in enumerate(poses):      # the chain's score order
            if cls[0] == 'chain' and cls[2] == 'A':
                vals = sorted((score[q], score[q + 1], score[q + 2]), reverse=True)
                who = {0: 'ABC', 1: 'BAC', 2: 'CBA'}[cls[1]]
                for name_, val in zip(who, vals):
                    score[q + 'ABC'.index(name_)] = val
        for q in order_idx:
            x, y2, box, cls = poses[q]
            p3.append(x)
            p2.append(y2)
            bx.append(list(box) + [score[q]])
            classes.append(cls)
        row_start.append(row_start[-1] + len(poses))
    return dict(index=i, J=J, A=A, J_model=Jm, skeleton=skeleton, order_by_score=order, var_correction=varc, alt=alt,
                params=params, edges=[tuple(e) for e in edges], mean_bones=mean_bones, counts=counts,
                row_start=row_start, classes=classes, poses3d=np.stack(p3).astype(F32), poses2d=np.stack(p2).astype(F32),
                boxes=np.array(bx, F32))


_CASES = {}


def case(i):
    if i not in _CASES:
        _CASES[i] = build_case(i)
    return _CASES[i]


def cases():
    return [case(i) for i in range(N_CASES)]


def sub_case(c, image):
    """Image `image` of the call as a call of its own."""
    lo, hi = c['row_start'][image], c['row_start'][image + 1]
    return dict(c, counts=[hi - lo], row_start=[0, hi - lo], classes=c['classes'][lo:hi], poses3d=c['poses3d'][lo:hi],
                poses2d=c['poses2d'][lo:hi], boxes=c['boxes'][lo:hi])


def torch_inputs(c, dtype):
    """(boxes, poses3d, poses2d, edges inside J_model, mean_bones) as cpu_ref.filter_poses takes them."""
    import torch
    rs = c['row_start']
    split = lambda x: [torch.from_numpy(x[a:b]).to(dtype) for a, b in zip(rs[:-1], rs[1:])]
    inside = [r for r, (a, b) in enumerate(c['edges']) if a < c['J_model'] and b < c['J_model']]
    return (split(c['boxes']), split(c['poses3d']), split(c['poses2d']), [c['edges'][r] for r in inside],
            torch.from_numpy(c['mean_bones'][inside]))


# ------------------------------------------------------------------------------------------------ the launch

def filter_params(c, **override):
    from metrabs_amd import _lib
    p = dict(c['params'], **override)
    return _lib.FilterParams(p['rel_small'], p['rel_big'], p['abs_diff_mm'], p['stdev_mm'], p['box_fraction'],
                             p['sim_scale_mm'], p['sim_threshold'], int(p['max_output']), int(c['var_correction']),
                             int(c['order_by_score']))


def run(lib, c, device='cuda'):
    """One mtr_filter_poses call through ctypes, in the manner of tests/test_gpu_filter.py::
    test_filter_refusals_guard_bands_and_repeats: `valid`, `keep_idx` and `keep_count` inside guard bands, the workspace
    the caller's own with a NaN prefill.  -> dict(valid, keep_idx, keep_count, mean [P, J, 3] f32, sim: per image its
    n_i^2 workspace floats, bands: the guard bands are intact, code)."""
    import ctypes

    import torch
    from metrabs_amd import _lib
    P, A, J = c['poses3d'].shape[:3]
    counts = [b - a for a, b in zip(c['row_start'][:-1], c['row_start'][1:])]
    dev = torch.device(device)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dt).to(dev)
    p3, p2, bx = t(c['poses3d'], torch.float32), t(c['poses2d'], torch.float32), t(c['boxes'], torch.float32)
    row_start = torch.tensor(c['row_start'], dtype=torch.int32, device=dev)
    offs = [sum(n * n for n in counts[:i]) for i in range(len(counts))]
    sim_off = torch.tensor(offs, dtype=torch.int32, device=dev)
    nb = len(c['edges'])
    e = torch.tensor(c['edges'], dtype=torch.int32, device=dev) if nb else None
    mb = t(c['mean_bones'], torch.float32) if nb else None
    need = lib.mtr_filter_poses_workspace_bytes(P, J, max(counts))
    assert need == (P * J * 3 + P * max(counts)) * 4
    ws = torch.full((need // 4 + 2,), float('nan'), dtype=torch.float32, device=dev)
    valid = torch.full((GUARD + P + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    keep_idx = torch.full((GUARD + P + GUARD,), -77, dtype=torch.int32, device=dev)
    keep_count = torch.full((GUARD + len(counts) + GUARD,), -77, dtype=torch.int32, device=dev)
    fp = filter_params(c)
    p = lambda x, off=0: ctypes.c_void_p(x.data_ptr() + off) if x is not None else None
    code = lib.mtr_filter_poses(p(p3), p(p2), p(bx), p(row_start), p(sim_off), len(counts), P, A, J, p(e), p(mb), nb,
                                c['J_model'], ctypes.byref(fp), p(ws), need, max(counts), p(valid, GUARD),
                                p(keep_idx, GUARD * 4), p(keep_count, GUARD * 4), _lib.current_stream_ptr(dev))
    torch.cuda.synchronize()
    bands = all(bool((x[:GUARD] == v).all()) and bool((x[len(x) - GUARD:] == v).all())
                for x, v in ((valid, 0x5A), (keep_idx, -77), (keep_count, -77)))
    w = ws.cpu().numpy()
    bands = bands and bool(np.isnan(w[need // 4:]).all())
    sim = [w[P * J * 3 + o:P * J * 3 + o + n * n].copy() for o, n in zip(offs, counts)]
    # (the workspace between the last image's block and its end, P * max_n - sum n_i^2 floats, is nobody's)
    rest = w[P * J * 3 + sum(n * n for n in counts):need // 4]
    bands = bands and bool(np.isnan(rest).all())
    return dict(code=code, valid=valid[GUARD:GUARD + P].cpu().numpy(), keep_idx=keep_idx[GUARD:GUARD + P].cpu().numpy(),
                keep_count=keep_count[GUARD:GUARD + len(counts)].cpu().numpy(), mean=w[:P * J * 3].reshape(P, J, 3).copy(),
                sim=sim, bands=bands)
