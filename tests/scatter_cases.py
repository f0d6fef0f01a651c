"""Test helpers of the table-gradient scatter (subgnn_amd/csrc/scatter.hip through ``ops.scatter_add_rows``, ``ops._GradAcc.flush``
and ``ops.sort_edges_by_key``): the seeded calls tests/test_gpu_scatter.py makes, the operation written out in float64 torch on the
CPU, and a restatement of the launch rules of scatter.hip / ops.py so that tests/test_scatter_cases_host.py can say without a GPU
which kernel instantiation each call reaches and which branches of the carry protocol its sorted keys walk through.  torch-CPU
only; nothing here reads the GPU or imports the package.

The operation:  table[k] += sum over the edges e with key_e == k != 0 of (c1_e * G[row(e)] + c2_e * v),  row(e) = edge_row[e] or
e // edges_per_row; c1 absent = 1, c2 absent = 0.  In ``arg`` mode (the max aggregator's backward) it is, per column d,
table[k, d] += sum over the DISTINCT rows r that list k of G[r, d] * [arg[r, d] == k]: a member listed twice counts once.  The op
ADDS: some cases of every family start from a table that is not zero.  Row 0 (PAD) is never touched.

Two kinds of values:
    float   randn: compared within helpers.REL_TOL and a norm bound.
    grid    every entry of G, c1, c2, v and of the initial table is an integer in [-2, 2] held in float32.  Every contribution
            and every partial sum is then an integer; ``inputs`` adds up |c1| |G| + |c2| |v| per target element on top of the
            initial |value| and REQUIRES the total to stay below 2^24, so a float32 evaluation in ANY order equals the float64
            one bit for bit (tests/test_scatter_cases_host.py shows it for every case) and the device result is compared with
            torch.equal: one dropped or doubled edge is seen however long the segment next to it is."""
import functools
from collections import namedtuple

import torch

# ---- the constants the launch rules depend on (tests/test_scatter_cases_host.py reads them out of scatter.hip / ops.py) ----------
RUN = 64                                # SC_RUN: sorted positions per wavefront ...
RUN_SMALL = 16                          # SC_RUN_SMALL: ... of launches of up to
SMALL_EDGES = 65536                     # SC_SMALL_EDGES edges
AHEAD = 8                               # SC_AHEAD: links the chain kernel requests together
MAXC = 4                                # SC_MAXC: columns per lane
MAX_D = 64 * MAXC                       # ops.SCATTER_MAX_D
LARGE_RUNS = 8192                       # more runs than this: D <= 64 without arg keeps 8 rows in flight, not the whole run
ONE_WG = 8192                           # SC_ONE_WG: keys the one-workgroup sort takes
IPTS = (1, 2, 3, 4, 5, 6, 8)            # its items-per-lane forms (1024 lanes)
MAX_JOBS = 40                           # SC_MAX_JOBS: lists per pack launch of sgnn_scatter_add_rows_multi
TOGETHER_BELOW = 1 << 16                # ops.SCATTER_TOGETHER_BELOW: shorter lists wait for the accumulator's flush
GRID_MAX = 2
EXACT_BELOW = 1 << 24                   # integers below are exact in float32

CHAIN_RUNS = (1, AHEAD, AHEAD + 1, 2 * AHEAD + 1)      # whole runs a constructed hub fills after a partial one = links of its chain
LAST_CHAIN_RUNS, LAST_CNT = 2, 1                       # the final hub: 2 whole runs, then a last run of 1 edge (E = 524289 is reachable)


# ---- the launch rules, restated ------------------------------------------------------------------------------------------------
def run_len(E):
    """sc_run_len."""
    return RUN_SMALL if E <= SMALL_EDGES else RUN


def n_runs(E):
    return (E + run_len(E) - 1) // run_len(E)


def form(E, D, arg=False, multi=False):
    """The scatter_runs_kernel<AHEAD, MAXC, RUN, MULTI> that sgnn_scatter_add_rows_sorted (sgnn_scatter_add_rows_multi for
    ``multi``, E = all lists' edges) launches."""
    if D > MAX_D:
        raise ValueError('unsupported width')
    r = run_len(E)
    if r == RUN_SMALL:
        a, c = (RUN_SMALL, 1) if D <= 64 else (RUN_SMALL, 2) if D <= 128 else (8, 4)
    elif D <= 64 and not arg and not multi:
        a, c = (64, 1) if n_runs(E) <= LARGE_RUNS else (8, 1)
    else:
        a, c = (16, 1) if D <= 64 else (16, 2) if D <= 128 else (8, 4)
    return (a, c, r, bool(multi))


def waits_for_flush(E, D, presorted=False, arg=False):
    """ops.scatter_add_rows(together=acc): the list only joins the accumulator's pending lists."""
    return E > 0 and not presorted and not arg and E < TOGETHER_BELOW and D <= MAX_D


def pack_launches(list_sizes):
    """Lists per scatter_pack_kernel launch of sgnn_scatter_add_rows_multi (lists without edges never reach it: ops drops them)."""
    sizes = [n for n in list_sizes if n > 0]
    return [len(sizes[lo:lo + MAX_JOBS]) for lo in range(0, len(sizes), MAX_JOBS)]


def sort_ipt(n):
    """Items per lane of sort_one_wg_kernel; None: rocPRIM's device sort."""
    if n > ONE_WG:
        return None
    return next(i for i in IPTS if n <= 1024 * i)


def key_bits(max_key):
    """sc_key_bits."""
    b = 1
    while b < 31 and (1 << b) <= max_key:
        b += 1
    return b


def classify(sk, run, ahead, rows=None):
    """What scatter_runs_kernel / scatter_chains_kernel do with the ascending keys ``sk`` at this run length: per run the
    head / tail flags it writes, where its first and last segment go, the chains (start run, links, run of the last link),
    the AHEAD groups whose source rows are not read (their last key is PAD), and -- with ``rows``, the source row of every
    sorted position (arg mode) -- the repeats of a member that a run boundary splits."""
    sk = sk.to(torch.int64)
    E = sk.numel()
    nr = (E + run - 1) // run
    p0 = torch.arange(nr) * run
    pend = torch.clamp(p0 + run, max=E)
    minus = torch.tensor([-1])
    first, last = sk[p0], sk[pend - 1]
    prev = torch.cat([minus, sk[p0[1:] - 1]])
    nxt = torch.cat([sk[pend[:-1]], minus])
    single = first == last
    from_prev = (first == prev) & (first != 0)
    first_on = single & (first == nxt) & (first != 0)
    head = from_prev.long() + 2 * (from_prev & first_on).long()
    tail = (~from_prev & first_on) | (~single & (last == nxt))
    owned_first = (first != 0) & ~from_prev & ~first_on
    owned_last = ~single & (last != nxt)
    changes = torch.zeros(E, dtype=torch.bool)
    changes[1:] = sk[1:] != sk[:-1]
    inner = changes.clone()
    inner[p0] = False
    segs = torch.zeros(nr, dtype=torch.int64).index_add_(0, torch.arange(E) // run, inner.long()) + 1
    chains = []
    hl = head.tolist()
    for t in tail.nonzero().view(-1).tolist():
        n, j = 0, t + 1
        while j < nr and hl[j] & 1:
            n += 1
            if not hl[j] & 2:
                break
            j += 1
        chains.append((t, n, min(j, nr - 1)))
    j0 = torch.arange(0, run, ahead).view(1, -1)
    cnt = (pend - p0).view(-1, 1)
    valid = j0 < cnt
    at = torch.minimum(p0.view(-1, 1) + j0 + ahead - 1, pend.view(-1, 1) - 1).clamp_(min=0)
    skipped = valid & (sk[at] == 0)
    out = {
        'n_runs': nr, 'head': head, 'tail': tail, 'chains': chains, 'last_cnt': int(pend[-1] - p0[-1]),
        'dest': {name for name, hit in (('head', (head == 1).any()), ('run-on', (head == 3).any()), ('tail', tail.any()),
                                        ('owned', (owned_first | owned_last | (segs > 2)).any()), ('pad', (first == 0).any()))
                 if bool(hit)},
        'head_and_tail': int(((head == 1) & tail & ~single).sum()),              # two different keys carried by one run
        'tail_then_segments_then_head': int(((head == 1) & tail & (segs > 2)).sum()),
        'boundary_on_run_end': int(changes[p0[1:]].sum()),
        'skipped_groups': int(skipped.sum()),
        'skipped_then_read': int((skipped.any(1) & (valid & ~skipped).any(1)).sum()),
        'pad_run_then_pad_start': int(((last[:-1] == 0) & (first[1:] == 0) & (last[1:] != 0)).sum()),
        'pad_run_exact': int(((last[:-1] == 0) & (first[1:] != 0)).sum()),
    }
    if rows is not None:
        rows = rows.to(torch.int64)
        p = p0[1:]
        same_key = (sk[p] == sk[p - 1]) & (sk[p] != 0)
        out['split_repeats'] = int((same_key & (rows[p] == rows[p - 1])).sum())
        q = p[p + 1 < E]
        out['repeat_after_other_row'] = int(((sk[q] == sk[q - 1]) & (sk[q] != 0) & (rows[q] != rows[q - 1])
                                             & (sk[q + 1] == sk[q]) & (rows[q + 1] == rows[q])).sum())
        inside = torch.ones(E, dtype=torch.bool)
        inside[p0] = False
        rep = torch.zeros(E, dtype=torch.bool)
        rep[1:] = (sk[1:] == sk[:-1]) & (sk[1:] != 0) & (rows[1:] == rows[:-1])
        out['repeats_inside'] = int((rep & inside).sum())
    return out


# ---- cases ----------------------------------------------------------------------------------------------------------------------
# family 'forms' | 'boundaries' | 'arg' | 'multi'; kind 'grid' | 'float'; spec: the family's own description (below); table0:
# the table starts from values that are not zero.
Case = namedtuple('Case', 'name family kind D spec table0 seed', defaults=(False, 0))
Forms = namedtuple('Forms', 'E rows terms')                 # rows 'div' (e // edges_per_row) | 'list' (edge_row); terms 'G' | 'v' | 'both'
Bounds = namedtuple('Bounds', 'E_min pad rows')             # pad: PAD prefix as a difference to the run length (0, -1, +1)
Arg = namedtuple('Arg', 'sets rows')                        # sets: rows of ARG_SLOTS entries; rows 'div' | 'list'
Multi = namedtuple('Multi', 'sizes')                        # edges per list
ARG_SLOTS = 5

FORM_SIZES = (1, 15, 16, 17, 65536, 65537)
FORM_SIZES_D64 = (524288, 524289)


def _cases():
    out = []
    # ---- forms: the smallest sizes on both sides of every threshold ----
    for E in FORM_SIZES:
        out.append(Case('forms-%d-D64' % E, 'forms', 'grid', 64, Forms(E, 'div', 'both'), table0=E in (17, 65537)))
    for E in (17, 65537):                                   # every addressing x term set at one small and one large form
        for rows in ('div', 'list'):
            for terms in ('G', 'v', 'both'):
                if (rows, terms) != ('div', 'both'):
                    out.append(Case('forms-%d-D64-%s-%s' % (E, rows, terms), 'forms', 'grid', 64, Forms(E, rows, terms)))
    out.append(Case('forms-524288-D64', 'forms', 'grid', 64, Forms(524288, 'list', 'G')))
    out.append(Case('forms-524289-D64', 'forms', 'grid', 64, Forms(524289, 'div', 'both'), table0=True))
    out.append(Case('forms-524289-D8', 'forms', 'grid', 8, Forms(524289, 'div', 'G')))
    out.append(Case('forms-65537-D8', 'forms', 'grid', 8, Forms(65537, 'list', 'both')))
    for D in (128, 200, 256):
        out.append(Case('forms-9100-D%d' % D, 'forms', 'grid', D, Forms(9100, 'list' if D == 128 else 'div', 'both' if D == 128 else 'v')))
        out.append(Case('forms-65536-D%d' % D, 'forms', 'grid', D, Forms(65536, 'div', 'G')))
        out.append(Case('forms-65537-D%d' % D, 'forms', 'grid', D, Forms(65537, 'list' if D == 200 else 'div', 'both'), table0=D == 256))
    # ---- boundaries: constructed key layouts at both run lengths, every instantiation that takes no arg ----
    for tag, E_min, Ds in (('run16', 0, (64, 128, 256)), ('run64', SMALL_EDGES + 1, (8, 128, 200)), ('run64-large', 524289, (64,))):
        for D in Ds:
            for pad in (0, -1, 1):
                if tag == 'run64-large' and pad != -1:
                    continue
                out.append(Case('boundaries-%s-D%d-pad%+d' % (tag, D, pad), 'boundaries', 'grid', D,
                                Bounds(E_min, pad, 'list' if pad == 1 else 'div'), table0=pad == 0))
    # ---- arg: repeated members inside a run and split by a run boundary ----
    for tag, sets, Ds in (('small', 400, (64, 128, 256)), ('large', 13200, (64, 128, 200))):
        for D in Ds:
            for rows in ('div', 'list'):
                if rows == 'list' and D != 64:
                    continue
                out.append(Case('arg-%s-D%d-%s' % (tag, D, rows), 'arg', 'grid', D, Arg(sets, rows), table0=rows == 'list'))
    # ---- multi: several lists into one table through ops._GradAcc ----
    for D in (64, 128, 200):
        out.append(Case('multi-3x30000-D%d' % D, 'multi', 'grid', D, Multi((30000, 30000, 30000)), table0=D == 128))
        out.append(Case('multi-empty-list-between-D%d' % D, 'multi', 'grid', D, Multi((500, 0, 700, 17, 1))))
    out.append(Case('multi-41-lists-D64', 'multi', 'grid', 64, Multi(tuple(40 + 13 * (k % 7) for k in range(MAX_JOBS + 1))), table0=True))
    # ---- one float twin per family and launch form ----
    seen, twins = set(), []
    for c in out:
        key = (c.family, case_form(c))
        if key not in seen and spec_edges(c) > 1:
            seen.add(key)
            twins.append(c._replace(name=c.name + '-float', kind='float'))
    return tuple(c._replace(seed=i + 1) for i, c in enumerate(out + twins))


def spec_edges(case):
    s = case.spec
    if case.family == 'forms':
        return s.E
    if case.family == 'arg':
        return s.sets * ARG_SLOTS
    if case.family == 'multi':
        return sum(s.sizes)
    return _layout(run_len(max(s.E_min, 1)), s.pad, s.E_min)[1]


def case_form(case):
    return form(spec_edges(case), case.D, arg=case.family == 'arg', multi=case.family == 'multi')


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
def _layout(R, pad, E_min):
    """(segments [(key, edges)] in ascending key order without the filler, E, filler edges, keys the filler may use): a PAD prefix
    of R + pad edges; a segment that ends exactly at a run end; for w in CHAIN_RUNS a hub that starts 3 edges before a run
    end, fills w whole runs and ends at a run end (a chain of w links, all but the last running on); a hub over one whole run
    and 5 edges of the next, two whole segments and the first R - 10 edges of another hub in that run (head carry and tail
    carry of two keys); random filler; the largest key starts 3 edges before a run end and ends LAST_CNT edges into the last run."""
    segs, pos = [(0, R + pad)], R + pad

    def add(n):
        nonlocal pos
        segs.append((len(segs), n))
        pos += n
    add((-pos) % R or R)
    for w in CHAIN_RUNS:
        add(R - 3)
        add(3 + w * R)
    add(R + 5)
    add(2)
    add(3)
    add(R - 10 + 4)
    add(R - 4)
    assert pos % R == 0
    last = 3 + LAST_CHAIN_RUNS * R + LAST_CNT
    filler = R - 3 + 4 * R
    while pos + filler + last < E_min:
        filler += R * max(1, (E_min - pos - filler - last) // R)
    return segs, pos + filler + last, filler, last


def _draw_values(g, kind, *shape):
    if kind == 'grid':
        return torch.randint(-GRID_MAX, GRID_MAX + 1, shape, generator=g).to(torch.float32)
    return torch.randn(*shape, generator=g)


def _list(g, kind, keys, D, rows, terms, per_row):
    """One edge list: its keys with source rows, coefficients and v as ``rows`` / ``terms`` say."""
    E = keys.numel()
    R = max(1, (E + per_row - 1) // per_row)
    d = {'keys': keys.to(torch.int32), 'G': None, 'edge_row': None, 'edges_per_row': per_row, 'c1': None, 'c2': None, 'v': None, 'arg': None}
    if terms != 'v':
        d['G'] = _draw_values(g, kind, R, D)
        if rows == 'list':
            d['edge_row'] = torch.randint(0, R, (E,), generator=g).to(torch.int32)
    if terms == 'both':
        d['c1'] = _draw_values(g, kind, E)
    if terms != 'G':
        d['c2'], d['v'] = _draw_values(g, kind, E), _draw_values(g, kind, D)
    return d


def _random_keys(g, E, n_rows, hub=11, hub_share=0.2, pad_share=0.1):
    keys = torch.randint(1, n_rows, (E,), generator=g)
    keys[torch.rand(E, generator=g) < hub_share] = hub
    keys[torch.rand(E, generator=g) < pad_share] = 0
    return keys


def _forms_inputs(case, g):
    s = case.spec
    n_rows = 50 if s.E < 100 else 3000
    keys = _random_keys(g, s.E, n_rows) if s.E > 1 else torch.tensor([7])
    return n_rows, [_list(g, case.kind, keys, case.D, s.rows, s.terms, 3 if s.E < 100 else 13)]


def _boundaries_inputs(case, g):
    s = case.spec
    R = run_len(max(s.E_min, 1))
    segs, E, filler, last = _layout(R, s.pad, s.E_min)
    assert run_len(E) == R
    n_rows = 2000
    fill = torch.sort(torch.randint(100, n_rows - 1, (filler,), generator=g))[0]
    sk = torch.cat([torch.repeat_interleave(torch.tensor([k for k, _ in segs]), torch.tensor([n for _, n in segs])), fill,
                    torch.full((last,), n_rows - 1)])
    assert sk.numel() == E
    keys = sk[torch.randperm(E, generator=g)]                # the sort has work to do
    return n_rows, [_list(g, case.kind, keys, case.D, s.rows, 'both', 7)]


def _arg_inputs(case, g):
    """Sets of ARG_SLOTS member ids.  With R the run length: P = R - 1 (mod R) PAD entries, then key 1 listed twice by set 0 and
    once by R - 2 later sets (its repeat is split by the run boundary), key 2 listed by set 1, twice by set 2 and by R - 3
    later sets (the run ends in key 2 of another set, the repeat opens the next run), key 3 three times by set 3 and by R - 4
    later sets (1 | 2 split), key 4 three times by set 4 (2 | 1 split); set 5 repeats two members inside a run."""
    s = case.spec
    A, S = ARG_SLOTS, s.sets
    E = S * A
    R = run_len(E)
    n_rows = 300 if S < 1000 else 3000
    sets = torch.randint(10, n_rows, (S, A), generator=g)
    fixed = torch.zeros(S, A, dtype=torch.bool)

    def put(row, ids):
        sets[row, :len(ids)] = torch.tensor(ids)
        fixed[row, :len(ids)] = True
    put(0, [1, 1])
    put(1, [2])
    put(2, [2, 2])
    put(3, [3, 3, 3])
    put(4, [4, 4, 4])
    put(5, [20, 21, 20, 21, 20])
    row = 10
    for key, others in ((1, R - 2), (2, R - 3), (3, R - 4), (4, 5)):
        for _ in range(others):
            put(row, [key])
            row += 1
    free = (~fixed).view(-1).nonzero().view(-1)
    P = (E // 10) // R * R + R - 1
    sets.view(-1)[free[torch.randperm(free.numel(), generator=g)[:P]]] = 0
    slot = torch.randint(0, A, (S, case.D), generator=g)
    d = {'keys': sets.view(-1).to(torch.int32), 'G': _draw_values(g, case.kind, S, case.D), 'edges_per_row': A, 'c1': None, 'c2': None,
         'v': None, 'edge_row': (torch.arange(E) // A).to(torch.int32) if s.rows == 'list' else None,
         'arg': torch.gather(sets, 1, slot).to(torch.int32)}
    return n_rows, [d]


MULTI_KINDS = (('div', 'both'), ('div', 'v'), ('list', 'G'), ('div', 'G'))       # list k is of kind k % 4


def _multi_inputs(case, g):
    n_rows = 3000
    lists = []
    for k, E in enumerate(case.spec.sizes):
        rows, terms = MULTI_KINDS[k % 4]
        lists.append(_list(g, case.kind, _random_keys(g, E, n_rows), case.D, rows, terms, 7))
    return n_rows, lists


def source_rows(d):
    E = d['keys'].numel()
    return d['edge_row'].long() if d['edge_row'] is not None else torch.arange(E) // d['edges_per_row']


def evaluate(case, inp, dtype, reverse=False, absolute=False):
    """The table after the case's lists, in ``dtype`` on the CPU; ``reverse``: every list's edges are added last first;
    ``absolute``: with |.| of every input -- a bound on the sum of the contributions' magnitudes."""
    conv = (lambda t: t.to(dtype).abs()) if absolute else (lambda t: t.to(dtype))
    table = conv(inp['table0']).clone()
    D = table.shape[1]
    for d in inp['lists']:
        keys, rows = d['keys'].long(), source_rows(d)
        if keys.numel() == 0:
            continue
        if d['arg'] is not None:
            code = torch.unique(rows * table.shape[0] + keys)                     # a member listed twice by a set counts once
            rows, keys = code // table.shape[0], code % table.shape[0]
            contrib = conv(d['G'])[rows] * (d['arg'].long()[rows] == keys.view(-1, 1)).to(dtype)
        else:
            if d['G'] is not None:
                contrib = conv(d['G'])[rows]
                if d['c1'] is not None:
                    contrib *= conv(d['c1']).view(-1, 1)
            else:
                contrib = torch.zeros(keys.numel(), D, dtype=dtype)
            if d['c2'] is not None:
                contrib += conv(d['c2']).view(-1, 1) * conv(d['v']).view(1, -1)
        live = keys != 0
        keys, contrib = keys[live], contrib[live]
        if reverse:
            keys, contrib = keys.flip(0), contrib.flip(0)
        table.index_add_(0, keys, contrib)
    return table


def _last_edge_counts(d):
    """Whether the edge that sorts last (the one edge of a boundaries layout's last run: the last link of the largest key's
    chain) adds something in some column -- a chain kernel that loses it must be seen."""
    e = int((d['keys'] == d['keys'].max()).nonzero()[-1])
    c = d['c1'][e].double() * d['G'][int(source_rows(d)[e])].double() + d['c2'][e].double() * d['v'].double()
    return bool((c != 0).any())


@functools.lru_cache(maxsize=2)
def inputs(case):
    """The CPU inputs of a case: {'n_rows', 'table0' (n_rows, D) float32, 'lists': [{'keys' int32 (E), 'G' (R, D) or None,
    'edge_row' int32 (E) or None, 'edges_per_row', 'c1', 'c2', 'v', 'arg' int32 (R, D) or None}]}.  Never modified.  boundaries:
    the first of the seeds 100 seed, 100 seed + 1, ... at which the one edge of the last run adds something."""
    for t in range(100):
        g = torch.Generator().manual_seed(100 * case.seed + t)
        n_rows, lists = {'forms': _forms_inputs, 'boundaries': _boundaries_inputs, 'arg': _arg_inputs, 'multi': _multi_inputs}[case.family](case, g)
        if case.family != 'boundaries' or _last_edge_counts(lists[0]):
            break
    else:
        raise ValueError('%s: no seed gives the last run a contribution that is not 0' % case.name)
    table0 = _draw_values(g, case.kind, n_rows, case.D) if case.table0 else torch.zeros(n_rows, case.D)
    inp = {'n_rows': n_rows, 'table0': table0, 'lists': lists}
    if case.kind == 'grid':
        bound = float(evaluate(case, inp, torch.float64, absolute=True).max())
        assert bound < EXACT_BELOW, '%s: a sum of magnitudes reaches %g: float32 is not exact there' % (case.name, bound)
    return inp


@functools.lru_cache(maxsize=2)
def reference(case):
    """``evaluate`` in float64."""
    return evaluate(case, inputs(case), torch.float64)


def sorted_view(d):
    """(ascending keys, source row of every sorted position) of a list, by a stable sort as sgnn_sort_edges_by_key's."""
    sk, order = torch.sort(d['keys'].long(), stable=True)
    return sk, source_rows(d)[order]


def classification(case):
    """``classify`` of the case's sorted keys (multi: of all lists' keys as one list) at the instantiation it reaches."""
    lists = [d for d in inputs(case)['lists'] if d['keys'].numel()]
    a, _, r, _ = case_form(case)
    if case.family == 'arg':
        sk, rows = sorted_view(lists[0])
        return classify(sk, r, a, rows)
    return classify(torch.sort(torch.cat([d['keys'].long() for d in lists]), stable=True)[0], r, a)


MUTATIONS = ('drop_last_link', 'last_row')


def emulate(case, mutate=None):
    """The table of a single-list case as the two kernels build it, in float64: every piece -- a stretch of one key inside
    one run -- is summed and goes to the table, to its run's head slot or to its run's tail slot by ``flush``'s rules, then
    every tail walks its chain of heads.  Equal to ``reference`` when the rules are right.  ``mutate``: what a kernel with one
    line wrong would give -- 'drop_last_link': scatter_chains_kernel leaves out the last link of every chain; 'last_row':
    scatter_runs_kernel starts every run with last_row = -1, whatever the previous run ended in (arg mode)."""
    assert mutate in (None,) + MUTATIONS and case.family != 'multi'
    inp = inputs(case)
    d = inp['lists'][0]
    R = case_form(case)[2]
    sk, order = torch.sort(d['keys'].long(), stable=True)
    rows = source_rows(d)[order]
    E, D = sk.numel(), case.D
    run_start = torch.arange(0, E, R)
    if d['arg'] is not None:
        contrib = d['G'].double()[rows] * (d['arg'].long()[rows] == sk.view(-1, 1))
        repeat = torch.zeros(E, dtype=torch.bool)
        repeat[1:] = (sk[1:] == sk[:-1]) & (rows[1:] == rows[:-1])
        if mutate == 'last_row':
            repeat[run_start] = False
        contrib[repeat] = 0
    else:
        contrib = torch.zeros(E, D, dtype=torch.float64)
        if d['G'] is not None:
            contrib += d['G'].double()[rows] * (1.0 if d['c1'] is None else d['c1'].double()[order].view(-1, 1))
        if d['c2'] is not None:
            contrib += d['c2'].double()[order].view(-1, 1) * d['v'].double().view(1, -1)
    start = torch.zeros(E, dtype=torch.bool)
    start[1:] = sk[1:] != sk[:-1]
    start[run_start] = True
    first = start.nonzero().view(-1)                                    # per piece: its first and last sorted position
    last = torch.cat([first[1:], torch.tensor([E])]) - 1
    psum = torch.zeros(first.numel(), D, dtype=torch.float64).index_add_(0, torch.cumsum(start, 0) - 1, contrib)
    pkey, prun = sk[first], first // R
    prev_key = torch.where(first > 0, sk[(first - 1).clamp(min=0)], torch.tensor(-1))
    next_key = torch.where(last + 1 < E, sk[(last + 1).clamp(max=E - 1)], torch.tensor(-1))
    from_prev = (first % R == 0) & (pkey == prev_key)
    into_next = ((last % R == R - 1) | (last == E - 1)) & (pkey == next_key)
    live = pkey != 0
    head, tail, owned = live & from_prev, live & ~from_prev & into_next, live & ~from_prev & ~into_next
    table = inp['table0'].double().clone()
    table.index_add_(0, pkey[owned], psum[owned])
    nr = (E + R - 1) // R
    head_val = torch.zeros(nr, D, dtype=torch.float64)
    head_val[prun[head]] = psum[head]
    flag = torch.zeros(nr, dtype=torch.int64)
    flag[prun[head]] = 1 + 2 * into_next[head].long()
    flag = flag.tolist()
    for i in tail.nonzero().view(-1).tolist():
        links, j = [], int(prun[i]) + 1
        while j < nr and flag[j] & 1:
            links.append(j)
            if not flag[j] & 2:
                break
            j += 1
        if mutate == 'drop_last_link':
            links = links[:-1]
        table[pkey[i]] += psum[i] + head_val[links].sum(0)
    return table


CASES = _cases()


# ---- ops.sort_edges_by_key -------------------------------------------------------------------------------------------------------
SortCase = namedtuple('SortCase', 'n max_key fill')          # fill 'random' | 'max' (every key max_key) | 'zero'
SORT_SIZES = (1024, 1025, 2048, 2049, 3072, 3073, 5120, 5121, 6144, 6145, 7168, 7169)
SORT_MAX_KEYS = (1, 1023, 65535, (1 << 31) - 1)
SORT_CASES = tuple([SortCase(n, (999, 1_000_000, (1 << 31) - 1)[i % 3], 'random') for i, n in enumerate(SORT_SIZES)]
                   + [SortCase(n, m, fill) for m in SORT_MAX_KEYS for fill in ('max', 'zero') for n in (1000, 8191)])


def sort_keys(case):
    g = torch.Generator().manual_seed(case.n)
    if case.fill == 'max':
        return torch.full((case.n,), case.max_key, dtype=torch.int32)
    if case.fill == 'zero':
        return torch.zeros(case.n, dtype=torch.int32)
    keys = torch.randint(0, min(case.max_key, 5000) + 1, (case.n,), generator=g).to(torch.int32)
    keys[torch.rand(case.n, generator=g) < 0.05] = case.max_key
    return keys
