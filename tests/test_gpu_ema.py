"""-m gpu: the weight average inside the fused Adam step (sgnn_optim_adam_ema / _ema_lr_table, optim.ClipAdam(ema_decay=)) and the
in-place exchange of parameters and averages (sgnn_optim_swap, ClipAdam.swap_ema).

Decays are 0.5 and 0.9, never 0.999: over six steps 0.999 leaves the average within tolerance of its initial value and a kernel
that never wrote it would pass.  Every case also asserts that the average has moved away from the initial values AND from the
current parameters by more than 100 x the tolerance.

Tolerance of the average, max|a - b| / max|b| < 1e-6 against the float64 recurrence e <- e + w (p - e) on the optimizer's own
parameters (which the existing tests pin to torch): six steps of at most 1.5 ulp of float32 rounding per fused lerp (the
difference, the fma), 6 x 1.5 x 6e-8 ~ 5e-7."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-6

NAMED = [1, 2, 3, 5, 64, 127, 1000, 4096, 4097, 70001]


def _sizes():
    g = torch.Generator().manual_seed(11)
    return [(1003, 64)] + [(n,) for n in NAMED] + [(int(x),) for x in torch.randint(1, 3000, (139,), generator=g)]


def _make(init):
    """Parameters on the device, every third one a view 4 bytes past a 16-byte boundary (the scalar path)."""
    out = []
    for i, t in enumerate(init):
        if i % 3 == 2:
            base = torch.zeros(t.numel() + 1, device=DEV)
            view = base[1:].view(t.shape)
            view.copy_(t)
            assert view.data_ptr() % 16 == 4
            out.append(torch.nn.Parameter(view))
        else:
            out.append(torch.nn.Parameter(t.clone().to(DEV)))
    return out


def _rel(a, b):
    """max|a - b| / max|b| (float64)."""
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _decay(d, warmup, s):
    return min(d, (1.0 + s) / (10.0 + s)) if warmup else d


def _ema(opt, p):
    return opt.state[id(p)]['ema']


# -- 1. every path and launch group against the float64 recurrence --------------------------------------------------------------
@pytest.mark.parametrize('capturable', [False, True])
@pytest.mark.parametrize('max_norm', [None, 0.7])
@pytest.mark.parametrize('d,warmup', [(0.5, False), (0.9, False), (0.9, True)])
def test_average_follows_the_recurrence_and_leaves_the_step_alone(capturable, max_norm, d, warmup):
    """150 tensors (the 72-tensor group bound of the bare update and the 56 of the averaging one are both crossed): a 1003 x 64
    table (row-skip path), sizes 1 .. 70 001 (float4 body, scalar tails, several workgroups), every third tensor unaligned,
    gradients missing on some steps (those tensors' step counts fall behind and their averages stay as they are)."""
    from subgnn_amd import optim
    shapes = _sizes()
    assert len(shapes) == 150
    g = torch.Generator().manual_seed(5)
    init = [torch.randn(*s, generator=g) for s in shapes]
    plain, avg = _make(init), _make(init)
    kw = dict(lr=0.01, max_norm=max_norm, big_bytes=1003 * 64 * 4, capturable=capturable)
    o_plain = optim.ClipAdam(plain, **kw)
    o_avg = optim.ClipAdam(avg, ema_decay=d, ema_warmup=warmup, **kw)
    assert len(o_avg.big) == 2 and o_avg.tail.seen and o_avg.param_groups[0]['ema_decay'] == d      # (the table and the 70 001)
    for p, t in zip(avg, init):
        assert torch.equal(_ema(o_avg, p).cpu(), t)                     # initialised to the parameter
    want = [t.double().to(DEV) for t in init]                          # the recurrence, in float64
    counts = [0] * len(shapes)
    for it in range(6):
        grads = [torch.randn(*s, generator=g) * (3.0 if it % 2 else 0.05) for s in shapes]
        grads[0][torch.rand(1003, generator=g) < 0.5] = 0               # rows without a gradient
        has = [not ((i % 7 == 3 and it in (1, 2)) or (i == 9 and it == 3)) for i in range(len(shapes))]
        for ps in (plain, avg):
            for p, gr, h in zip(ps, grads, has):
                p.grad = gr.to(DEV) if h else None
        before = [_ema(o_avg, p).clone() for p, h in zip(avg, has) if not h]
        o_plain.step(); o_avg.step()
        o_plain.zero_grad(); o_avg.zero_grad()
        errs = []
        for i, (p, h) in enumerate(zip(avg, has)):
            if h:
                counts[i] += 1
                w = 1.0 - _decay(d, warmup, counts[i])
                want[i] = want[i] + w * (p.detach().double() - want[i])
            errs.append((_ema(o_avg, p).double() - want[i]).abs().max() / want[i].abs().max().clamp_min(1e-30))
        errs = torch.stack(errs).cpu()
        worst = int(errs.argmax())
        print('step %d: worst average error %.3g (tensor %d, %s)' % (it, float(errs[worst]), worst, shapes[worst]))
        assert float(errs[worst]) < TOL, (it, worst, shapes[worst], float(errs[worst]))
        for e0, (p, h) in zip(before, [(p, h) for p, h in zip(avg, has) if not h]):
            assert torch.equal(_ema(o_avg, p), e0)                      # no step, no move
    for i, (a, b) in enumerate(zip(avg, plain)):
        assert torch.equal(a.detach(), b.detach()), i
        for name in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(o_avg.state[id(a)][name], o_plain.state[id(b)][name]), (i, name)
        e = _ema(o_avg, a)
        assert _rel(e, init[i].to(DEV)) > 100 * TOL and _rel(e, a) > 100 * TOL, (i, shapes[i])
    by_id = dict(zip((id(p) for p in o_avg.all), o_avg.counters.tolist())) if capturable else {id(p): o_avg.state[id(p)]['step'] for p in avg}
    steps = [by_id[id(p)] for p in avg]
    assert steps == counts and counts[0] == 6 and counts[3] == 4 and counts[9] == 5


# -- 2. skipped rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('poison', [False, True])
@pytest.mark.parametrize('D', [4, 64, 256, 48])
def test_average_of_skipped_rows_is_bit_exact(D, poison):
    """A row the update skips never had a gradient: its average equals its parameter bit for bit and e + w (p - e) leaves it
    as it is, so the average with skipping == the average of the dense update, and never-touched rows hold the initial bits.
    ``poison``: a NaN gradient at step 2 -- the NaN clip coefficient steps every row, and every average turns NaN with its
    parameter."""
    from subgnn_amd import optim
    g = torch.Generator().manual_seed(D)
    rows = 5001
    init = [torch.randn(rows, D, generator=g), torch.randn(D, 7, generator=g)]
    models = [[torch.nn.Parameter(t.clone().to(DEV)) for t in init] for _ in range(2)]
    kw = dict(lr=0.01, max_norm=0.5, big_bytes=rows * D * 4, ema_decay=0.5)
    o_skip = optim.ClipAdam(models[0], **kw)
    o_dense = optim.ClipAdam(models[1], skip_untouched_rows=False, **kw)
    assert (len(o_skip.tail.seen) == 1) == (D != 48) and not o_dense.tail.seen
    touched = torch.zeros(rows, dtype=torch.bool)
    for it in range(6):
        pick = torch.rand(rows, generator=g) < (0.0 if it == 3 else 0.15)           # step 3: no row at all
        pick[0] = False
        touched |= pick
        gt = torch.randn(rows, D, generator=g) * pick.unsqueeze(1)
        gs = torch.randn(D, 7, generator=g)
        if poison and it == 2:
            gs[3, 2] = float('nan')
        for ps in models:
            ps[0].grad, ps[1].grad = gt.clone().to(DEV), gs.clone().to(DEV)
        o_skip.step(); o_dense.step()
        o_skip.zero_grad(); o_dense.zero_grad()
        for k in range(2):
            if not (poison and it >= 2):                                            # (NaN != NaN)
                assert torch.equal(_ema(o_skip, models[0][k]), _ema(o_dense, models[1][k])), (it, k)
                assert torch.equal(models[0][k], models[1][k]), (it, k)
        if poison and it == 2:
            for ps, opt in zip(models, (o_skip, o_dense)):
                for p in ps:
                    assert bool(torch.isnan(p).all()) and bool(torch.isnan(_ema(opt, p)).all())
            return
    never = ~touched.to(DEV)
    e = _ema(o_skip, models[0][0])
    assert torch.equal(e[never].cpu(), init[0][~touched])                           # the initial bits
    seen = touched.to(DEV)
    assert _rel(e[seen], init[0].to(DEV)[seen]) > 100 * TOL and _rel(e[seen], models[0][0][seen]) > 100 * TOL


# -- 3. the exchange ------------------------------------------------------------------------------------------------------------
def test_swap_exchanges_parameters_and_averages_in_place():
    """Aligned and unaligned tensors, scalar tails, several launch groups (150 + 1 tensors, 128 per launch), an empty tensor:
    one swap_ema() makes the parameters bit-equal to the former averages and the other way round, in the same storage; a second
    one restores both; step() raises in between."""
    from subgnn_amd import optim
    shapes = _sizes() + [(0,)]
    g = torch.Generator().manual_seed(9)
    init = [torch.randn(*s, generator=g) for s in shapes]
    ps = _make(init)
    opt = optim.ClipAdam(ps, lr=0.01, max_norm=0.7, big_bytes=1003 * 64 * 4, ema_decay=0.9)
    for k, p in enumerate(ps):                          # averages of their own; some of them unaligned while their parameter is not
        if k % 5 == 1 and p.numel():
            base = torch.zeros(p.numel() + 1, device=DEV)
            opt.state[id(p)]['ema'] = base[1:].view(p.shape)
        _ema(opt, p).copy_(torch.randn(*p.shape, generator=g))
    opt.ema = [opt.state[id(p)]['ema'] for p in opt.all]
    p0, e0 = [p.detach().clone() for p in ps], [_ema(opt, p).clone() for p in ps]
    ptrs = [p.data_ptr() for p in ps]
    opt.swap_ema()
    assert opt.swapped
    for p, a, b in zip(ps, p0, e0):
        assert torch.equal(p.detach(), b) and torch.equal(_ema(opt, p), a)
    assert [p.data_ptr() for p in ps] == ptrs
    for p in ps:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match='exchanged'):
        opt.step()
    opt.swap_ema()
    assert not opt.swapped
    for p, a, b in zip(ps, p0, e0):
        assert torch.equal(p.detach(), a) and torch.equal(_ema(opt, p), b)
    opt.step()                                          # (and steps again)
    with pytest.raises(ValueError, match='ema_decay'):
        optim.ClipAdam(_make(init[:3]), lr=0.01).swap_ema()


# -- 4. a recorded step ---------------------------------------------------------------------------------------------------------
def test_scheduled_averaging_step_replays_from_a_hipgraph():
    """One eager step, then the scheduled + averaging step recorded into a hipGraph and replayed four times == five eager steps,
    bit for bit: parameters, moments, averages (the rate and the warm-up decay follow the device step count)."""
    from subgnn_amd import optim
    g = torch.Generator().manual_seed(12)
    shapes = [(300, 16), (70001,), (640,), (3,), (129,)]
    init = [torch.randn(*s, generator=g) for s in shapes]
    table = torch.tensor([1e-2, 3e-2, 7e-3, 2e-2, 5e-3], dtype=torch.float32, device=DEV)
    sets = []
    for _ in range(2):
        ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
        sets.append((ps, optim.ClipAdam(ps, lr=0.5, max_norm=0.3, big_bytes=4096, capturable=True, lr_schedule=table,
                                        ema_decay=0.5, ema_warmup=True)))
    (got, o_got), (ref, o_ref) = sets
    assert o_got.tail.seen
    grads = []
    for it in range(5):
        gr = [torch.randn(*s, generator=g) * (2.0 if it == 2 else 0.1) for s in shapes]
        gr[0][torch.rand(300, generator=g) < 0.6] = 0
        grads.append([x.to(DEV) for x in gr])
    static = [x.clone() for x in grads[0]]
    for p, sg in zip(got, static):
        p.grad = sg
    o_got.step()                                                       # (one eager step)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        with torch.cuda.graph(graph, stream=stream):
            for p, sg in zip(got, static):
                p.grad = sg
            o_got.step()
    torch.cuda.current_stream().wait_stream(stream)
    assert o_got.counters.tolist() == [1] * 5                          # recording runs nothing
    for it in range(1, 5):
        for sg, gr in zip(static, grads[it]):
            sg.copy_(gr)
        graph.replay()
    for it in range(5):
        for p, gr in zip(ref, grads[it]):
            p.grad = gr.clone()
        o_ref.step()
    torch.cuda.synchronize()
    assert o_got.counters.tolist() == [5] * 5 == o_ref.counters.tolist()
    for k, (a, b) in enumerate(zip(got, ref)):
        assert torch.equal(a.detach(), b.detach()), k
        for name in ('exp_avg', 'exp_avg_sq', 'ema'):
            assert torch.equal(o_got.state[id(a)][name], o_ref.state[id(b)][name]), (k, name)
        assert _rel(_ema(o_got, a), init[k].to(DEV)) > 100 * TOL and _rel(_ema(o_got, a), a) > 100 * TOL


# -- 5. the optimizer's state -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('capturable', [False, True])
def test_state_round_trip_carries_the_average(capturable):
    """state_dict -> a fresh ClipAdam -> load_state_dict continues bit for bit, averages included; a state without 'ema' starts
    the average at the loaded parameters."""
    from subgnn_amd import optim
    g = torch.Generator().manual_seed(5)
    rows, D = 3001, 32
    init = [torch.randn(rows, D, generator=g), torch.randn(D, 9, generator=g), torch.randn(D, generator=g)]

    def fresh():
        ps = [torch.nn.Parameter(t.clone().to(DEV)) for t in init]
        return ps, optim.ClipAdam(ps, lr=0.01, max_norm=0.5, big_bytes=rows * D * 4, capturable=capturable, ema_decay=0.9,
                                  ema_warmup=True)

    def run(ps, opt, its):
        for it in its:
            gg = torch.Generator().manual_seed(100 + it)
            pick = (torch.rand(rows, generator=gg) < 0.1).unsqueeze(1)
            pick[0] = False
            for p, gr in zip(ps, [torch.randn(rows, D, generator=gg) * pick, torch.randn(D, 9, generator=gg), torch.randn(D, generator=gg)]):
                p.grad = gr.to(DEV)
            opt.step()
            opt.zero_grad()
    a_ps, a = fresh()
    run(a_ps, a, range(5))
    b_ps, b = fresh()
    run(b_ps, b, range(3))
    sd = b.state_dict()
    assert sd['param_groups'][0]['ema_decay'] == 0.9 and sd['param_groups'][0]['ema_warmup'] is True
    assert all('ema' in e for e in sd['state'].values())
    assert 'ema' in b.state_refs()['state'][0] and b.state_refs()['state'][0]['ema'] is _ema(b, b_ps[0])      # live, not a copy
    c_ps, c = fresh()
    for p, q in zip(c_ps, b_ps):
        p.data.copy_(q.data)
    c.load_state_dict(sd)
    for p, q in zip(c_ps, b_ps):
        assert torch.equal(_ema(c, p), _ema(b, q)) and _rel(_ema(c, p), p) > 100 * TOL
    run(c_ps, c, range(3, 5))
    for p, q in zip(c_ps, a_ps):
        assert torch.equal(p.detach(), q.detach())
        for name in ('exp_avg', 'exp_avg_sq', 'ema'):
            assert torch.equal(c.state[id(p)][name], a.state[id(q)][name]), name
    # without the averages (a state saved by a run that kept none): they start at the loaded parameters
    d_ps, d_opt = fresh()
    for p, q in zip(d_ps, b_ps):
        p.data.copy_(q.data)
    bare = {'state': {k: {n: v for n, v in e.items() if n != 'ema'} for k, e in sd['state'].items()},
            'param_groups': [{k: v for k, v in sd['param_groups'][0].items() if k not in ('ema_decay', 'ema_warmup')}]}
    d_opt.load_state_dict(bare)
    assert d_opt.ema_decay == 0.9
    for p, q in zip(d_ps, b_ps):
        assert torch.equal(_ema(d_opt, p), q.detach())
    run(d_ps, d_opt, range(3, 5))
    for p, q in zip(d_ps, a_ps):
        assert torch.equal(p.detach(), q.detach()) and not torch.equal(_ema(d_opt, p), p.detach())
