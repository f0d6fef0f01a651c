"""Test helpers of the fastdtw kernels (structure_similarity_fn = 'dtw', subgnn_amd/csrc/dtw.hip): a restatement of what
``sgnn_dtw_similarity`` launches for a pair -- which kernel, which instantiation, which form every level of the pair runs
through -- and the seeded cases tests/test_gpu_dtw_paths.py runs, so that tests/test_dtw_paths_host.py can say without a GPU
which paths those cases reach.  Numpy only; nothing here reads the GPU."""
import os

import numpy as np

GOLDEN_RULES = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dtw_rules.npz')
TIES = (0, 1, 2)

# ---- the dispatch of dtw.hip, restated ------------------------------------------------------------------------------------------
# (the kernel's own condition is quoted behind each line: compare with dtw_run and dtw_similarity_reg_kernel)
DTW_R = 32                              # #define DTW_R 32
DTW_NT = 256 * 512                      # DTW_THREADS * DTW_BLOCKS: lanes of the general kernel's launch
DTW_REG_WAVES = 256 * (256 * 32) // 64  # DTW_REG_NT / 64: wavefronts of the register kernel's launch (32 768)
PYR_WAVE_MAX_SERIES, PYR_WAVE_MAX_LEN = 8192, 1024      # DTW_PYR_WAVE_MAX_SERIES, DTW_PYR_WAVE_MAX_LEN
WORKSPACE_CAP = 2 << 30                 # no case may ask for more workspace than this


def words_in_lds(max_y):
    """dtw_words_in_lds: ``(max_y_len >> 1) * DTW_THREADS * 4 <= 48 * 1024`` -- true up to max_y_len 97."""
    return (max(max_y, 1) >> 1) * 256 * 4 <= 48 * 1024


def rmax_of(max_x):
    """dtw_run: ``if (max_x_len <= 12) ... else if (max_x_len <= 20) ... else`` (32)."""
    return 12 if max_x <= 12 else (20 if max_x <= 20 else 32)


def n_levels(lx, ly):
    """``n_levels = 1; while (lx >= 3 && ly >= 3) { lx >>= 1; ly >>= 1; ++n_levels; }`` -- 0 for a pair with an empty row."""
    if lx == 0 or ly == 0:
        return 0
    n = 1
    while lx >= 3 and ly >= 3:
        lx, ly, n = lx >> 1, ly >> 1, n + 1
    return n


def _chunks(ly):
    """``for (jc = 0; jc < ly; jc += 64)`` in the level functions (the row-major form has one table: at most 32 columns): 1, 2
    or 3+ chunks of the hull table."""
    c = (ly + 63) // 64
    return '3+' if c >= 3 else str(c)


def level_form(rmax, wlds, lev, ly):
    """The function level ``lev`` of a pair runs through in dtw_similarity_reg_kernel<RMAX, TIE, MINB, WLDS>; ``ly`` is the
    level's column count ``ly0 >> lev``."""
    if lev == 0:
        return 'finest'                                  # if (lev == 0) dtw_wave_level<RMAX, TIE, WLDS, true>
    rh = ((rmax // 2) + 1) & ~1                          # constexpr int RH = ((RMAX / 2) + 1) & ~1
    if not 2 * rh <= 27:                                 # else if constexpr (2 * RH <= 27) ... else
        return 'coarse32'                                #     dtw_wave_level<RH, TIE, WLDS, false>   (RMAX 32: RH 16)
    if wlds and ly <= 32:                                # if (WLDS && ly <= 32): dtw_wave_level_2col<RH / R2 / R3, TIE, WLDS, true>
        return 'rm-RH' if lev == 1 else ('rm-R2' if lev == 2 else 'rm-R3')      # lev == 1 / lev == 2 / else
    return 'pp-lds' if wlds else 'pp-global'             # else dtw_wave_level_2col<RH, TIE, WLDS, false>


def pair_labels(max_x, max_y, kernel, ly, lx):
    """Path labels of ONE pair: an x row of ``lx`` entries against a y row of ``ly`` in a call that states ``max_x`` /
    ``max_y`` and asks for ``kernel``."""
    if not (max_x <= DTW_R and kernel == 0):             # const bool use_reg = max_x_len <= DTW_R && kernel == 0
        return {'general'} if n_levels(lx, ly) else {'general', 'general/empty'}
    rmax, wlds = rmax_of(max_x), words_in_lds(max_y)
    inst = 'reg/RMAX%d/WLDS%d' % (rmax, wlds)
    out = {inst}
    if n_levels(lx, ly) == 0:
        out.add('reg/empty')
    for lev in range(n_levels(lx, ly)):
        out.add('%s/%s/chunks%s' % (inst, level_form(rmax, wlds, lev, ly >> lev), _chunks(ly >> lev)))
    return out


def call_labels(max_x, max_y, kernel, x_lens, y_lens, ordered=False):
    """Path labels of a whole call: its pairs' (over the distinct pairs of lengths), the pyramid kernels of both sides and
    whether the DP kernel's grid-stride loop wraps."""
    x_lens, y_lens = np.asarray(x_lens), np.asarray(y_lens)
    n_x, n_y = len(x_lens), len(y_lens)
    out = set()
    for lx in np.unique(x_lens):
        for ly in np.unique(y_lens):
            out |= pair_labels(max_x, max_y, kernel, int(ly), int(lx))
    use_reg = max_x <= DTW_R and kernel == 0
    # dtw_launch_pyramid: if (n <= DTW_PYR_WAVE_MAX_SERIES && M <= DTW_PYR_WAVE_MAX_LEN) wave kernel, else one thread per series
    # x: transposed = 1, order = use_reg ? x_order : nullptr;  y: transposed = 0, no order
    x_form = 'wave' if n_x <= PYR_WAVE_MAX_SERIES and max_x <= PYR_WAVE_MAX_LEN else 'thread'
    y_form = 'wave' if n_y <= PYR_WAVE_MAX_SERIES and max_y <= PYR_WAVE_MAX_LEN else 'thread'
    out.add('pyr/x/%s%s' % (x_form, '+order' if ordered and use_reg else ''))
    out.add('pyr/y/%s' % y_form)
    if use_reg:
        if ((n_x + 63) // 64) * n_y > DTW_REG_WAVES:     # for (task = wave0; task < n_tasks; task += n_waves), n_tasks = chunks * n_y
            out.add('reg/grid-stride')
    elif n_x * n_y > DTW_NT:                             # for (pair = tid; pair < total; pair += NT)
        out.add('general/grid-stride')
    return out


def required_labels():
    """Every label of the dispatch that a call with max_y_len <= 200 can reach: 6 register instantiations per rule with the
    forms and chunk counts their coarse levels can take, the general kernel, both grid-stride loops, six pyramid forms."""
    out = {'general', 'general/empty', 'general/grid-stride', 'reg/empty', 'reg/grid-stride',
           'pyr/x/wave', 'pyr/x/wave+order', 'pyr/x/thread', 'pyr/x/thread+order', 'pyr/y/wave', 'pyr/y/thread'}
    for rmax in (12, 20, 32):
        for wlds in (True, False):
            inst = 'reg/RMAX%d/WLDS%d' % (rmax, wlds)
            out.add(inst)
            # the finest level has up to 97 columns with the words in LDS (two chunks), 98+ otherwise (three from 129)
            forms = [('finest', ('1', '2') if wlds else ('1', '2', '3+'))]
            if rmax == 32:
                forms.append(('coarse32', ('1',) if wlds else ('1', '2')))       # level 1 of a y row of 130+ entries: 65+ columns
            elif wlds:
                forms += [('rm-RH', ('1',)), ('rm-R2', ('1',)), ('rm-R3', ('1',)), ('pp-lds', ('1',))]
            else:
                forms.append(('pp-global', ('1', '2')))
            out |= {'%s/%s/chunks%s' % (inst, f, c) for f, cs in forms for c in cs}
    return out


# ---- the mined fixture (tests/golden/make_goldens_dtw_rules.py) ---------------------------------------------------------------

MIN_RULE_PAIRS = 16


class RuleCell:
    """One cell of dtw_rules.npz: x rows of one length class, y rows of one length class, the oracle's three matrices."""

    def __init__(self, name, xs, ys, sims):
        self.name, self.xs, self.ys, self.sims = name, xs, ys, sims
        (x_lo, x_hi), (y_lo, y_hi) = (tuple(int(v) for v in part[1:].split('_')) for part in name.split('__'))
        self.x_class, self.y_class = (x_lo, x_hi), (y_lo, y_hi)

    def calls(self):
        """(max_x, max_y, kernel) of every call the rows are sent through: the instantiation their lengths select and the
        general kernel, then the same data with ``max_x_len`` / ``max_y_len`` overstated -- the arguments choose the
        instantiation, not the data: 12-row data also through the 20- and 32-row forms and the general kernel (40), every y
        class also with its predecessor words' place decided by max_y_len 97 (where the rows fit) and 130."""
        x_hi, y_hi = self.x_class[1], self.y_class[1]
        max_xs = [(m, 0) for m in (12, 20, 32) if m >= x_hi] + [(max(x_hi, 40), 0)]
        if x_hi <= 32:
            max_xs.append((x_hi, 1))                      # the general kernel at the natural size
        max_ys = [m for m in (65, 97, 130) if m >= y_hi]
        return [(mx, my, k) for mx, k in max_xs for my in max_ys]


def load_rule_cells():
    z = np.load(GOLDEN_RULES, allow_pickle=False)

    def rows(kind):
        ends = np.cumsum(z[kind + '_len'].astype(np.int64))
        return [z[kind + '_val'][e - n:e].astype(np.int32).tolist() for e, n in zip(ends, z[kind + '_len'])]
    xs, ys = rows('x'), rows('y')
    cells = []
    for k, name in enumerate(str(n) for n in z['cells']):
        cells.append(RuleCell(name, [x for x, c in zip(xs, z['x_cell']) if c == k], [y for y, c in zip(ys, z['y_cell']) if c == k],
                              [z['%s_tie%d' % (name, t)] for t in TIES]))
    return cells


# ---- the length-boundary sweep -------------------------------------------------------------------------------------------------

SWEEP_MAX_X = (1, 2, 3, 11, 12, 13, 19, 20, 21, 31, 32, 33, 70)
# level counts change at 3 / 6 / 12 / 24 / 48; 65 starts a second column chunk and is the last row-major size (level 1 has 32
# columns for 64 and 65, 33 for 66); 97 is the last size with the words in LDS; 129 starts a third chunk, 130 a chunked level 1
SWEEP_Y_LENS = (1, 2, 3, 5, 6, 7, 11, 12, 13, 23, 24, 25, 47, 48, 49, 63, 64, 65, 66, 67, 96, 97, 127, 128, 129, 130, 131)
SWEEP_N_X = 231                         # 3 wavefronts and 39 rows: not a multiple of 64
INT_MAX = 2 ** 31 - 1


def _values(rng, n, regime, sort):
    """Three regimes: 0 = values below 6 (many ties); 1 = heavy-tailed "degrees" up to 2e5; 2 = small values with entries
    near 2^31 - 1 among them (the reciprocal path with large operands, costs near 2e9)."""
    if regime == 0:
        v = rng.integers(0, 6, n)
    elif regime == 1:
        v = np.minimum(rng.pareto(0.6, n) * 3.0, 2e5).astype(np.int64)
    else:
        v = rng.integers(0, 6, n)
        big = rng.random(n) < 0.4
        v[big] = INT_MAX - rng.integers(0, 1000, int(big.sum()))
    if sort:
        v = np.sort(v)
    return [int(t) for t in v]


def sweep_rows(max_x):
    """(xs, ys) of the sweep at ``max_x``: x rows of every length 0..max_x (a sample of them above 33), then random lengths,
    SWEEP_N_X rows in all, interleaved by length as listed (a wavefront holds rows of 0, 1, 2, 3, ... entries: different level
    counts, dissimilar series); row k is of regime k % 3, sorted when (k // 3) is even.  y rows: SWEEP_Y_LENS in each regime,
    sorted and unsorted alternating, and one empty row."""
    rng = np.random.default_rng(9000 + max_x)
    lens = list(range(max_x + 1)) if max_x <= 33 else [0, 1, 2, 3, 11, 12, 13, 20, 21, 32, 33, 34, 47, 48, 63, 64, 65, 69, 70]
    lens += [max_x] * 2
    while len(lens) < SWEEP_N_X:
        lens.append(int(rng.integers(0 if len(lens) % 29 == 0 else 1, max_x + 1)))
    xs = [_values(rng, n, k % 3, (k // 3) % 2 == 0) for k, n in enumerate(lens)]
    ys = [_values(rng, n, r, (k + r) % 2 == 0) for r in range(3) for k, n in enumerate(SWEEP_Y_LENS)]
    ys.append([])
    return xs, ys


def sweep_runs(max_x, ys):
    """(max_y, the y rows' indices) of the two runs at every max_x: max_y_len 97 over the rows that fit (predecessor words in
    LDS) and the true maximum over all of them (global scratch)."""
    fit = [k for k, y in enumerate(ys) if len(y) <= 97]
    return [(97, fit), (max(len(y) for y in ys), list(range(len(ys))))]


def sorted_row(row):
    return all(a <= b for a, b in zip(row, row[1:]))


# ---- grid-stride loops and pyramid forms ------------------------------------------------------------------------------------------

def _distinct(rng, n, lo, hi, bound=None):
    """n rows of lo..hi entries: values below ``bound``, or (None) of the sweep's regimes 0 and 1, sorted and unsorted."""
    out = []
    for k in range(n):
        m = int(rng.integers(lo, hi + 1))
        out.append([int(v) for v in rng.integers(0, bound, m)] if bound is not None else
                   _values(rng, m, 0 if k % 4 else 1, k % 2 == 0))
    return out


def big_case(name):
    """name -> dict(max_x, max_y, kernel, base_x, pick_x, base_y, pick_y, ordered): the call's x rows are base_x[pick_x], its y
    rows base_y[pick_y]; the oracle scores the distinct rows and the test gathers.
      reg-tasks      70 400 x rows against 32 y rows: 35 200 tasks for 32 768 wavefronts, and more than 8 192 series: the
                     one-thread-per-series pyramid kernel, transposed, with and without a processing order
      general-pairs  3 000 x rows of up to 40 entries against 50 y rows: 150 000 pairs for the general kernel's 131 072 lanes
      many-y         70 x rows against 8 200 y rows: the y side's one-thread-per-series pyramid kernel (not transposed)"""
    rng = np.random.default_rng({'reg-tasks': 31, 'general-pairs': 32, 'many-y': 33}[name])
    if name == 'reg-tasks':
        base_x = [[]] + _distinct(rng, 299, 1, 20)
        base_y = _distinct(rng, 32, 1, 50, 7)
        return dict(max_x=20, max_y=50, kernel=0, base_x=base_x, pick_x=rng.integers(0, 300, 70400), base_y=base_y,
                    pick_y=np.arange(32), ordered=(True, False))
    if name == 'general-pairs':
        base_x = [[]] + _distinct(rng, 499, 1, 40)
        base_y = [[]] + _distinct(rng, 49, 1, 60, 7)
        return dict(max_x=40, max_y=60, kernel=0, base_x=base_x, pick_x=rng.integers(0, 500, 3000), base_y=base_y,
                    pick_y=np.arange(50), ordered=(False,))
    base_x = [[]] + _distinct(rng, 69, 1, 12, 5)
    base_y = [[]] + _distinct(rng, 199, 1, 12, 5)
    return dict(max_x=12, max_y=12, kernel=0, base_x=base_x, pick_x=np.arange(70), base_y=base_y,
                pick_y=rng.integers(0, 200, 8200), ordered=(False,))


BIG_CASES = ('reg-tasks', 'general-pairs', 'many-y')

# ---- sgnn_dtw_similarity_live -------------------------------------------------------------------------------------------------------

LIVE_CASES = [(12, 50), (12, 130), (20, 50), (20, 130)]          # (max_x, max_y): RMAX 12 / 20, words in LDS / global scratch


def live_rows(max_x, max_y):
    """300 x rows of 0..max_x entries (about one in eight empty) drawn from 60 distinct ones, 23 y rows of 1..max_y entries, the
    longest first."""
    rng = np.random.default_rng(500 + max_x + max_y)
    base = [[int(v) for v in rng.integers(0, 6, 0 if k % 8 == 0 else int(rng.integers(1, max_x + 1)))] for k in range(60)]
    xs = [base[int(i)] for i in rng.integers(0, 60, 300)]
    ys = [[int(v) for v in rng.integers(0, 6, n)] for n in [max_y] + [int(v) for v in rng.integers(1, max_y + 1, 22)]]
    return xs, ys


# ---- every call of the GPU file, for the coverage test ------------------------------------------------------------------------------

def all_calls():
    """(name, ties, max_x, max_y, kernel, x lengths, y lengths, ordered) of every kind of call tests/test_gpu_dtw_paths.py makes
    against the oracle (repetitions through ops.dtw_similarity left out: they reach no label the raw call does not, except
    the processing order of rows, listed for the sweep)."""
    out = []
    for cell in load_rule_cells():
        xl, yl = [len(x) for x in cell.xs], [len(y) for y in cell.ys]
        for mx, my, k in cell.calls():
            out.append(('rules/%s/%d/%d/%d' % (cell.name, mx, my, k), TIES, mx, my, k, xl, yl, False))
    for max_x in SWEEP_MAX_X:
        xs, ys = sweep_rows(max_x)
        xl = [len(x) for x in xs]
        for max_y, idx in sweep_runs(max_x, ys):
            yl = [len(ys[k]) for k in idx]
            out.append(('sweep/%d/%d' % (max_x, max_y), TIES, max_x, max_y, 0, xl, yl, False))
            out.append(('sweep/%d/%d/ops' % (max_x, max_y), TIES, max_x, max_y, 0, xl * 5, yl, True))
        out.append(('sweep/%d/general' % max_x, TIES, max_x, max(len(y) for y in ys), 1, xl, [len(y) for y in ys], False))
    for name in BIG_CASES:
        c = big_case(name)
        xl = np.array([len(x) for x in c['base_x']])[c['pick_x']]
        yl = np.array([len(y) for y in c['base_y']])[c['pick_y']]
        for ordered in c['ordered']:
            out.append(('big/%s/%d' % (name, ordered), TIES, c['max_x'], c['max_y'], c['kernel'], xl, yl, ordered))
    for max_x, max_y in LIVE_CASES:
        xs, ys = live_rows(max_x, max_y)
        out.append(('live/%d/%d' % (max_x, max_y), TIES, max_x, max_y, 0, [len(x) for x in xs if x], [len(y) for y in ys], True))
    return out
