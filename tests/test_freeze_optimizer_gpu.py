"""The optimiser over a set of ranges (csrc/optim.hip: reed_grad_sqnorm_ranges, reed_adamw_ema_ranges) and FusedAdamWEMA on a partly
frozen model.  Kernel level: against reed_adamw_ema itself on a compacted copy (inside the ranges: the same bits), against the
untouched state (outside: the same bits) and against an fp64 norm; model level: against the fp64 restatement of clip_grad_norm_ /
AdamW / update_ema that tests/test_optimizer_gpu.py uses (restated here)."""
import copy
import math

import pytest
import torch

from tests.rowpass_ref import DTYPE, U, Guarded, bits

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS, WD, DECAY = 1e-2, 0.9, 0.999, 1e-8, 0.01, 0.99
SPAN = 8192 * 256 * 4                 # elements one lap of the update kernel's grid covers
N_TOTAL = SPAN + 4 * 3000             # not a multiple of the span: a second, short lap
N_TRAIN = N_TOTAL - 4 * 1000          # the pos_embed-style tail: EMA and shadow only
NB = 2048


def _many():
    """Several hundred ranges of uneven length and uneven gaps over the whole trained part, the second lap included."""
    out, at, k = [], 8, 0
    while at + 4 * 700 < N_TRAIN and len(out) < 400:
        n = 4 * (1 + (k * 37) % 611)
        out.append((at, at + n))
        at += n + 4 * (1 + (k * 101) % 5000)
        k += 1
    out.append((N_TRAIN - 64, N_TRAIN))
    return out


TABLES = {
    "one_vector": [(4 * 12345, 4 * 12345 + 4)],
    "from_zero": [(0, 4 * 1000)],
    "to_n_train": [(N_TRAIN - 4 * 777, N_TRAIN)],
    "adjacent": [(4 * 1000, 4 * 70000), (4 * 70000, 4 * 70100)],
    "merged": [(4 * 1000, 4 * 70100)],
    "inside_a_stride": [(SPAN + 40, SPAN + 48)],      # between two visits of one thread, in the short second lap
    "hundreds": _many(),
    "everything": [(0, N_TRAIN)],
}


@pytest.fixture(params=["bf16", "fp16"])
def build16(request, dev):
    from reed_amd import ops
    prev = ops.use(request.param)
    yield request.param
    ops.use(prev)


def randn(n, seed, dev, scale=1.0):
    return (torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale).to(dev)


@pytest.fixture(scope="module")
def base(dev):
    p = randn(N_TOTAL, 1, dev)
    return dict(p=p, ema=p + randn(N_TOTAL, 2, dev, 0.01), m=randn(N_TOTAL, 5, dev, 0.05), v=randn(N_TOTAL, 6, dev, 0.01) ** 2,
                g=randn(N_TOTAL, 3, dev, 0.1))


def mask_of(pairs, dev, n=N_TOTAL):
    m = torch.zeros(n, dtype=torch.bool, device=dev)
    for b, e in pairs:
        m[b:e] = True
    return m


def close(tag, got, ref, rtol=2e-6, atol=5e-7):
    """The project's tolerance for this update (tests/test_optimizer_gpu.py: fp32 FMA-contraction noise)."""
    err = (got.double() - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (atol + rtol * ref.abs()))
    r = float(torch.where(torch.isfinite(err), ratio, torch.full_like(err, float("inf"))).max())
    print(f"[adamw_ema_ranges] {tag}: worst error / (atol + rtol |ref|) = {r:.3f}")
    assert r <= 1.0, tag


def norm_budget_u(n_inside, nblocks):
    """Relative budget of the norm in units of u.  The reduction has the shape of reed_grad_sqnorm's (the union dealt vector by
    vector over 256 nblocks threads): per thread `laps` vectors x 5 roundings (four products folded into the sum, one add), 8 for
    the wave and block sums, the rest in fp64; every term is positive, so the sum is within (5 laps + 8) u relative; the square
    root halves that, its rounding to fp32 adds u / 2 (budgeted: a whole u)."""
    laps = max(1, -(-(n_inside // 4) // (256 * nblocks)))
    return (5 * laps + 8) / 2 + 1


# ------------------------------------------------------------------------------------------------------------ the norm
@pytest.mark.parametrize("name", list(TABLES))
def test_norm_over_ranges_reads_nothing_outside(dev, base, name):
    from reed_amd import ops
    pairs = TABLES[name]
    inside = mask_of(pairs, dev)
    g = torch.where(inside, base["g"], torch.full_like(base["g"], float("nan")))     # one stray read: a NaN norm
    rg = ops.Ranges(pairs, dev)
    for nblocks in (NB, 3):                                                          # idle blocks at 2048; many laps at 3
        partial = Guarded(nblocks, torch.float32, dev)
        ops.grad_sqnorm_ranges(g, rg, N_TRAIN, partial.t, nblocks)
        nc = Guarded(2, torch.float32, dev)
        ops.clip_finalize(partial.t, nblocks, 1.0, nc.t)
        torch.cuda.synchronize()
        assert partial.intact() and nc.intact() and not torch.isnan(partial.t).any(), "a partial was not written, or is NaN"
        ref = math.sqrt(float((base["g"][inside].double() ** 2).sum()))
        bud = norm_budget_u(int(inside.sum()), nblocks)
        r = abs(float(nc.t[0]) - ref) / (bud * U * ref)
        print(f"[norm over ranges {name} blocks={nblocks}] error / ({bud:.1f} u norm) = {r:.3f}")
        assert r <= 1.0, (float(nc.t[0]), ref)


def test_adjacent_ranges_equal_their_merged_form(dev, base):
    from reed_amd import ops
    out = []
    for name in ("adjacent", "merged"):
        partial = torch.empty(NB, device=dev)
        ops.grad_sqnorm_ranges(base["g"], ops.Ranges(TABLES[name], dev), N_TRAIN, partial, NB)
        out.append(partial)
    assert torch.equal(bits(out[0]), bits(out[1]))
    # ... and one range over everything is reed_grad_sqnorm's assignment: the same partials, bit for bit
    a, b = torch.empty(NB, device=dev), torch.empty(NB, device=dev)
    ops.grad_sqnorm_ranges(base["g"], ops.Ranges(TABLES["everything"], dev), N_TRAIN, a, NB)
    ops.grad_sqnorm(base["g"], N_TRAIN, b, NB)
    assert torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------- the update
class State:
    def __init__(self, base, dt, dev, n=N_TOTAL):
        self.g = {k: Guarded(n, torch.float32, dev) for k in ("p", "m", "v", "ema")}
        for k, gd in self.g.items():
            gd.t.copy_(base[k][:n])
        self.g["shadow"] = Guarded(n, dt, dev, fill=7.0)
        self.p, self.m, self.v, self.ema, self.shadow = (self.g[k].t for k in ("p", "m", "v", "ema", "shadow"))

    def intact(self):
        return all(gd.intact() for gd in self.g.values())


def ranged_step(ops, s, g, rg, nc=None, scaler=None, t=3):
    ops.adamw_ema_ranges(s.p, g, s.m, s.v, s.ema, s.shadow, N_TRAIN, N_TOTAL, nc, LR, B1, B2, EPS, WD, 1 - B1 ** t, 1 - B2 ** t,
                         DECAY, rg, scaler_state=scaler)


@pytest.mark.parametrize("name", list(TABLES))
def test_update_over_ranges(dev, build16, base, name):
    from reed_amd import ops
    dt = DTYPE[build16]
    pairs = TABLES[name]
    inside = mask_of(pairs, dev)
    g = torch.where(inside, base["g"], torch.full_like(base["g"], float("nan")))
    s = State(base, dt, dev)
    ranged_step(ops, s, g, ops.Ranges(pairs, dev))
    torch.cuda.synchronize()
    assert s.intact()
    # inside: reed_adamw_ema on a compacted copy of just those elements
    n_in = int(inside.sum())
    assert n_in % 4 == 0
    c = {k: base[k][inside].clone() for k in ("p", "m", "v", "g")}
    ops.adamw_ema(c["p"], c["g"], c["m"], c["v"], None, None, n_in, n_in, None, LR, B1, B2, EPS, WD, 1 - B1 ** 3, 1 - B2 ** 3, DECAY)
    # outside: untouched
    for k in ("p", "m", "v"):
        got = getattr(s, k)
        assert torch.equal(bits(got[inside]), bits(c[k])), f"{k} inside the ranges differs from reed_adamw_ema"
        assert torch.equal(bits(got[~inside]), bits(base[k][~inside])), f"{k} moved outside the ranges"
    assert not torch.equal(bits(s.p[inside]), bits(base["p"][inside]))
    # the EMA and the shadow: reed_adamw_ema's, everywhere (its EMA / shadow part alone on the updated p)
    ema, shadow = base["ema"].clone(), torch.empty(N_TOTAL, dtype=dt, device=dev)
    ops.adamw_ema(s.p.clone(), None, None, None, ema, shadow, 0, N_TOTAL, None, LR, B1, B2, EPS, WD, 0.1, 0.1, DECAY)
    assert torch.equal(bits(s.ema), bits(ema)) and torch.equal(bits(s.shadow), bits(shadow))
    assert torch.equal(bits(s.shadow), bits(s.p.to(dt)))


def test_update_chunk_by_chunk_on_offset_pointers(dev, build16, base):
    """The overlap path's form: one call per update chunk on offset pointers, each with the part of the table cut to the chunk."""
    from reed_amd import ops
    dt = DTYPE[build16]
    pairs = TABLES["hundreds"]
    whole = State(base, dt, dev)
    nc = torch.tensor([123.0, 0.25], device=dev)
    ranged_step(ops, whole, base["g"], ops.Ranges(pairs, dev), nc=nc)
    s = State(base, dt, dev)
    cut = 4 * (1000 * 256 + 77)
    chunks = [(0, cut), (cut, N_TRAIN + 400), (N_TRAIN + 400, N_TOTAL)]
    table, where = [], []
    for b, e in chunks:
        part = [(max(rb, b), min(re_, e)) for rb, re_ in pairs if rb < e and re_ > b]
        where.append((len(table), len(part)))
        table += part
    rg = ops.Ranges(table, dev)
    hb = s.shadow.element_size()
    for (b, e), (first, count) in zip(chunks, where):
        nt = max(0, min(e, N_TRAIN) - b)
        ptr = lambda x, w=4: x.data_ptr() + w * b   # noqa: E731
        ops.adamw_ema_ranges(ptr(s.p), ptr(base["g"]) if nt else None, ptr(s.m) if nt else None, ptr(s.v) if nt else None,
                             ptr(s.ema), ptr(s.shadow, hb), nt, e - b, nc, LR, B1, B2, EPS, WD, 1 - B1 ** 3, 1 - B2 ** 3, DECAY,
                             rg, offset=b, first=first, count=count)
    torch.cuda.synchronize()
    assert s.intact()
    for k in ("p", "m", "v", "ema", "shadow"):
        assert torch.equal(bits(getattr(s, k)), bits(getattr(whole, k))), k


def test_update_over_ranges_with_a_loss_scaler(dev, build16, base):
    from reed_amd import ops
    dt = DTYPE[build16]
    pairs = TABLES["hundreds"]
    inside = mask_of(pairs, dev)
    rg = ops.Ranges(pairs, dev)
    nc = torch.tensor([123.0, 0.25 / 1024], device=dev)
    gs = base["g"] * 1024
    # an overflowed step skips inside the ranges too; the EMA and the shadow still run
    s = State(base, dt, dev)
    ranged_step(ops, s, gs, rg, nc=nc, scaler=torch.tensor([1024.0, 0.0, 1.0, 0.0], device=dev))
    torch.cuda.synchronize()
    for k in ("p", "m", "v"):
        assert torch.equal(bits(getattr(s, k)), bits(base[k])), k
    assert not torch.equal(bits(s.ema), bits(base["ema"])) and torch.equal(bits(s.shadow), bits(base["p"].to(dt)))
    # a clean step: the plain kernel's bits inside (bias corrections from the steps taken), nothing outside
    st = torch.tensor([1024.0, 1.0, 0.0, 2.0], device=dev)
    s = State(base, dt, dev)
    ranged_step(ops, s, gs, rg, nc=nc, scaler=st, t=7)
    c = {k: base[k][inside].clone() for k in ("p", "m", "v")}
    n_in = int(inside.sum())
    ops.adamw_ema(c["p"], gs[inside].clone(), c["m"], c["v"], None, None, n_in, n_in, nc, LR, B1, B2, EPS, WD, 0.5, 0.5, DECAY,
                  scaler_state=st)
    torch.cuda.synchronize()
    for k in ("p", "m", "v"):
        assert torch.equal(bits(getattr(s, k)[inside]), bits(c[k])) and torch.equal(bits(getattr(s, k)[~inside]), bits(base[k][~inside])), k


def test_bad_tables_are_refused(dev):
    from reed_amd import ops
    n = 4096
    x = torch.full((n,), 7.0, device=dev)
    partial = torch.full((4,), 7.0, device=dev)
    bad = {"unsorted": [(64, 128), (0, 32)], "overlaps": [(0, 64), (32, 128)], "misaligned": [(2, 64)],
           "misaligned end": [(0, 62)], "past the end": [(0, 32), (n - 32, n + 32)], "empty": [(64, 64)],
           "at most": [(8 * k, 8 * k + 4) for k in range(ops.MAX_RANGES + 1)]}
    for what, pairs in bad.items():
        size = max(n, 8 * (ops.MAX_RANGES + 2))
        big = torch.full((size,), 7.0, device=dev) if what == "at most" else x
        rg = ops.Ranges(pairs, dev)
        match = {"misaligned end": "misaligned", "empty": "empty or reversed", "at most": "at most 1024"}.get(what, what)
        with pytest.raises(RuntimeError, match=match):
            ops.grad_sqnorm_ranges(big, rg, big.numel(), partial, 4)
        with pytest.raises(RuntimeError, match=match):
            ops.adamw_ema_ranges(big, big, big, big, None, None, big.numel(), big.numel(), None, LR, B1, B2, EPS, WD, 0.1, 0.1,
                                 DECAY, rg)
    # exactly the cap is fine
    size = 8 * ops.MAX_RANGES
    big = torch.ones(size, device=dev)
    ops.grad_sqnorm_ranges(big, ops.Ranges([(8 * k, 8 * k + 4) for k in range(ops.MAX_RANGES)], dev), size, partial, 4)
    torch.cuda.synchronize()
    assert float(partial.sum()) == 4.0 * ops.MAX_RANGES and (x == 7.0).all()


# --------------------------------------------------------------------------------------------------------- model level
def _model(dev, which="b_last_block_final"):
    from tests.test_freeze_model_gpu import apply_set
    from tests.test_model_gpu import build_hip_model
    from tests.test_oracle_golden import TINY_CASES
    m = build_hip_model(TINY_CASES["hd64"]["cfg"], dev, 11)
    on = apply_set(m, which) if which else {n for n, _ in m.named_parameters() if n != "pos_embed"}
    ema = copy.deepcopy(m).requires_grad_(False).eval()
    return m, ema, on


def _backward(m, dev):
    from tests.test_input_grad_model_gpu import hip_grads
    hip_grads(m, dev, "hd64", False, x_grad=False, t_grad=False)


@pytest.mark.parametrize("overlap", [False, True])
def test_two_steps_on_a_partly_frozen_model(dev, overlap):
    from reed_amd.optim import FusedAdamWEMA, update_ema
    m, ema, on = _model(dev)
    update_ema(ema, m, decay=0)
    opt = FusedAdamWEMA(m, ema, lr=LR, betas=(B1, B2), weight_decay=WD, eps=EPS, max_grad_norm=1.0, ema_decay=DECAY, overlap=overlap)
    assert opt.overlap == overlap
    A, L = m._arena, m._layout
    names = [n for n, _ in m.named_parameters() if n != "pos_embed"]
    p0 = {n: p.detach().clone() for n, p in m.named_parameters()}
    e0 = {n: p.detach().clone() for n, p in ema.named_parameters()}
    A.ensure_shadow("bf16")
    sh0 = A.shadow.clone()
    master0 = A.master.clone()
    ref = {n: dict(p=p0[n].double(), m=torch.zeros_like(p0[n]).double(), v=torch.zeros_like(p0[n]).double()) for n in on}
    e64 = {n: e0[n].double() for n in e0}
    for t in (1, 2):
        opt.zero_grad(set_to_none=True)
        _backward(m, dev)
        g = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
        assert set(g) == on
        opt.step()
        opt.flush()
        torch.cuda.synchronize()
        # the norm: of the trainable gradients only, within the kernel-level budget
        want = math.sqrt(sum(float((v.double() ** 2).sum()) for v in g.values()))
        got = float(opt.grad_norm)
        bud = norm_budget_u(sum(v.numel() for v in g.values()), 2048)
        print(f"[freeze optimiser overlap={overlap} step {t}] grad_norm {got:.6f}, fp64 {want:.6f}: error / ({bud} u) = "
              f"{abs(got - want) / (bud * U * want):.3f}")
        assert abs(got - want) <= bud * U * want
        clip = float(opt.norm_clip[1])
        assert 0 < clip <= 1
        for n in on:                                           # torch.optim.AdamW + clip_grad_norm_ in fp64
            r = ref[n]
            gg = g[n].double() * clip
            r["p"] = r["p"] * (1 - LR * WD)
            r["m"] = r["m"] + (1 - B1) * (gg - r["m"])
            r["v"] = r["v"] * B2 + (1 - B2) * gg * gg
            r["p"] = r["p"] - (LR / (1 - B1 ** t)) * (r["m"] / (r["v"].sqrt() / math.sqrt(1 - B2 ** t) + EPS))
        cur = dict(m.named_parameters())
        for n in e64:                                          # update_ema walks every parameter, frozen ones included
            e64[n] = e64[n] * DECAY + cur[n].detach().double() * (1 - DECAY)
    cur, cur_e = dict(m.named_parameters()), dict(ema.named_parameters())
    inside = torch.zeros(L.n_total, dtype=torch.bool, device=dev)
    for n in on:
        off = L.off(n)
        inside[off:off + L.numel(n)] = True
        o = slice(off, off + L.numel(n))
        close(f"{n} p", cur[n].detach().flatten(), ref[n]["p"].flatten())
        close(f"{n} exp_avg", opt.exp_avg[o], ref[n]["m"].flatten())
        close(f"{n} exp_avg_sq", opt.exp_avg_sq[o], ref[n]["v"].flatten(), rtol=2e-5, atol=0.0)
        assert not torch.equal(cur[n].detach(), p0[n])
    # frozen: master weights, moments and the 16-bit shadow keep their bits; the EMA is the decay lerp of the unchanged weight
    frozen = [n for n in names if n not in on]
    assert frozen
    for n in frozen:
        o = slice(L.off(n), L.off(n) + L.numel(n))
        assert torch.equal(bits(cur[n].detach()), bits(p0[n])), n
        assert not opt.exp_avg[o].any() and not opt.exp_avg_sq[o].any(), n
        assert torch.equal(bits(A.shadow[o]), bits(sh0[o])), n
    assert torch.equal(bits(A.master[~inside]), bits(master0[~inside]))
    for n in e64:
        close(f"ema {n}", cur_e[n].detach().flatten(), e64[n].flatten())
    assert torch.equal(bits(A.shadow), bits(A.master.to(torch.bfloat16)))


@pytest.mark.parametrize("overlap", [False, True])
def test_all_trainable_makes_the_old_calls(dev, overlap, monkeypatch):
    from reed_amd import ops
    from reed_amd.optim import FusedAdamWEMA
    calls = []
    for name in ("grad_sqnorm", "adamw_ema", "grad_sqnorm_ranges", "adamw_ema_ranges"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _f=fn, **k: (calls.append(_n), _f(*a, **k))[1])
    for which, ranged in ((None, False), ("b_last_block_final", True)):
        m, ema, _ = _model(dev, which)
        opt = FusedAdamWEMA(m, ema, lr=LR, max_grad_norm=1.0, overlap=overlap)
        del calls[:]
        _backward(m, dev)
        opt.step()
        opt.flush()
        torch.cuda.synchronize()
        want = {"grad_sqnorm_ranges", "adamw_ema_ranges"} if ranged else {"grad_sqnorm", "adamw_ema"}
        assert set(calls) == want, (which, calls)


def test_state_dict_omits_frozen_parameters_and_round_trips(dev):
    from reed_amd.optim import FusedAdamWEMA
    m, ema, on = _model(dev)
    opt = FusedAdamWEMA(m, ema, lr=LR, max_grad_norm=1.0)
    _backward(m, dev)
    opt.step()
    sd = opt.state_dict()
    names = [n for n, _ in m.named_parameters()]
    assert {names[i] for i in sd["state"]} == on and sd["param_groups"][0]["params"] == list(range(len(names)))
    opt2 = FusedAdamWEMA(m, ema, lr=1.0)
    opt2.load_state_dict(copy.deepcopy(sd))
    assert opt2.step_count == 1 and opt2.lr == LR
    assert torch.equal(bits(opt2.exp_avg), bits(opt.exp_avg)) and torch.equal(bits(opt2.exp_avg_sq), bits(opt.exp_avg_sq))
    sd2 = opt2.state_dict()
    assert sd2["state"].keys() == sd["state"].keys()
    assert all(torch.equal(sd2["state"][i]["exp_avg"], sd["state"][i]["exp_avg"]) for i in sd["state"])


def test_unfreezing_after_a_step_raises_and_freezing_is_fine(dev):
    from reed_amd.optim import FusedAdamWEMA
    m, ema, on = _model(dev)
    opt = FusedAdamWEMA(m, ema, lr=LR, max_grad_norm=1.0)
    _backward(m, dev)
    opt.step()
    m.final_layer.linear.weight.requires_grad_(False)          # freezing one more: fine
    before = m.final_layer.linear.weight.detach().clone()
    opt.zero_grad(set_to_none=True)
    _backward(m, dev)
    opt.step()
    torch.cuda.synchronize()
    assert torch.equal(bits(m.final_layer.linear.weight.detach()), bits(before))
    m.blocks[0].mlp.fc1.weight.requires_grad_(True)            # training what has missed a step: refused
    opt.zero_grad(set_to_none=True)
    _backward(m, dev)
    count = opt.step_count
    with pytest.raises(RuntimeError, match="became trainable"):
        opt.step()
    assert opt.step_count == count


def test_sharded_pass_refuses_a_partly_frozen_model(dev, monkeypatch):
    from reed_amd.optim import FusedAdamWEMA
    monkeypatch.setenv("REED_OPT_SHARD", "1")
    m, ema, _ = _model(dev)
    opt = FusedAdamWEMA(m, ema, lr=LR)
    _backward(m, dev)
    p0 = m._arena.master.clone()
    with pytest.raises(RuntimeError, match="REED_OPT_SHARD"):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(bits(m._arena.master), bits(p0))
