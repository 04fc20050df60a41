"""The cell table, fp64 reference, error budgets and fp32 restatements of the 16-bit attention kernels (csrc/attention.hip: eleven
kernels behind ops.attention_fwd, ops.attention_bwd (with and without a workspace) and ops.attention_bwd_dp).  A plain module, not
a test file, after the pattern of tests/gemm_ref.py: tests/test_attention_budgets_cpu.py proves the budgets on the CPU (every
restatement stays at or below 0.6 of them, every realistic bug leaves them by more than 20 times, the guard check sees a planted
write), tests/test_attention_ref_gpu.py holds every cell of the bf16 and the IEEE-half build to them.

THE TABLE (CELLS): one row per (entry, kernel reached, head_dim, T list, (B, H), knobs).  There is no host planner for attention:
`kernel` is documentation, read off reed_attention_fwd / reed_attention_bwd / attention_bwd_persistent at the bottom of
csrc/attention.hip, and `cond` quotes the dispatch condition that reaches it.  Every T carries the feature it is there for.  The
"item loop" rows run under ops.set_cu_reserve(224) — reed_num_cus never plans for fewer than 32 CUs, so the persistent grids are 32
workgroups — with (B, H) = (9, 11): 99 items, every workgroup walks three or four, the n + 1 / n + 2 prefetches and counted waits
are in steady state.  Everywhere else (B, H) is (2, 3) or smaller.  Not in the table, because no call reaches them in the
default build: attn_fwd256p_kernel<64, true> and <72, true> (T = 256 goes to attn_fwd256v_kernel unless the library is built with
-DREED_ATTN_FWD_VDB_DEFAULT=0) and the REED_ATTN_DIAG instantiations.

INPUTS (inputs()): seeded on the CPU, rounded to the build's type before the reference sees them; logical [B H, T, hd].  Flavours:
`unit` (q, k, v, dO ~ N(0, 1)), `peaked` (q, k x 2.5: near one-hot rows, where a wrong scale shows), and in the fp16 build for the
backward `small_do` (dO x 2**-14: dS and dV reach fp16 subnormals, the floor term holds them) and `big_do` (dO x 2**10, a
loss-scaled gradient that stays finite).  Every key has a positive column 0 (|k_0| + 1), which gives the last special row its
meaning.  SPECIAL ROWS in every item with T >= 8: row 1 a zero query (P uniform, lse = log T); rows 2 and 3 identical keys; row 4 a
query of 8 x the spread; row 5 the query -64 e_0, whose scores are all below -8 sqrt(64 / hd) (an unmasked phantom key of score 0
then dominates the row); row T - 1 — the last row of every item, the last one's too — the query 6 k_{T-1}, one-hot on the last
key (the last tile, the last wave).  The backward cells receive O = round16(O_exact) and lse = fp32(lse_exact) from the
reference, so they do not depend on the forward kernel; the dp cells receive dpart [H, S, B T] made here (S = 1 at hd 64, 2 at hd
72: columns below 64 of the head in slot 0, the rest in slot 1, fp64 sums rounded to fp32), which isolates the attention side
from GEMM epilogue 13 (tests/gemm_ref.py holds that).

BUFFERS (Band): every buffer a kernel is given is a slice of a larger allocation with NaN guard rows in front and behind, outputs
NaN-filled before the call; after it every guard element is still NaN and every live output element finite.

BUDGETS: bounds from the arithmetic (u = 2**-24 = rowpass_ref.U), never from what a kernel returns.  n = T + hd + 8, u' = 2 u (the
project's MFMA convention, gemm_ref.py: safe under truncation of every partial sum, UNMEASURED); v_exp_f32 and v_rcp_f32 count 1
ulp (embed_ref.py) and are inside n.
  * fp32 error of p: relative e_p = n u' (1 + |lse| + |s|) — the hd products and T additions behind s and l, the fma, the
    exponential, the fp32 rounding of lse the backward is handed.
  * a 16-bit-rounded p or dS: one whole ulp relative, ulp16 = 2**-(mantissa bits), plus the absolute floor of the type's subnormal
    spacing (2**-24 in fp16): for the forward's unnormalised p = exp(s - m) scaled by exp(m - lse) = 1 / l, as it is for the
    backward's p = exp(s - lse) itself.  Pe_ij = P_ij (ulp16 + e_p) + floor is the absolute bound of the rounded p_ij.
  * O: sum_j Pe_ij |v_jd|, plus (sum_j Pe_ij) |o_id| for the denominator, plus one ulp of the output type taken at |O| + the rest.
  * lse: n u' (1 + |lse| + max_j |s_ij|), plus 1 ulp of __logf's result (UNMEASURED; the GPU run stays inside with it, so no
    measurement of |__logf - log| was needed).  ONES cells: at hd 72 and T <= 256 the forward is attn_fwd256p_kernel<72> /
    attn_fwd256v_kernel<72> with ONES = true: column 72 of the V tile is set to 1.0, so the softmax denominator comes out of the PV
    product itself — it is the sum of the 16-bit-ROUNDED p, not of the fp32 ones.  l then carries one 16-bit ulp relative, which is
    its absolute size in the log: lse gets + ulp16 there.  (Legitimate: O is normalised by the sum of exactly the p it is built
    from.  The CPU experiment behind this work held that lse to the fp32 budget and missed it by 4.5 times.)
  * delta = sum_d dO_d O_d: sum_d |dO_d| |O16_d - O_d| — the kernel is given the ROUNDED O, the largest term of dS — plus the fp32
    dot's (hd + 1) u' sum_d |dO_d O16_d|.  That is the STATED form (reference(inp, stated=True)).  Its first term is no
    arithmetic of any kernel: it bounds D_i = sum_d dO_d (O16_d - O_d), a number the inputs fix, by the sum of the absolute values,
    and over a few thousand rows |D_i| reaches 0.75 of that bound — with a near one-hot row behind it the restatement, and any
    correct kernel, then sits at 0.6 .. 0.75 of the stated dQ budget whatever its own arithmetic does (measured: the peaked flavour
    of 24 backward cases).  So the tests use the SHARP form (the default): the reference takes delta = sum_d dO_d O16_d, the fp64
    value of what the kernel is asked to compute from the O it is given, and the budget drops the first term.  The sharp check
    implies the stated one (|got - ref_stated| <= |got - ref_sharp| + |ref_sharp - ref_stated|, and the dropped term bounds the
    second difference, which test_attention_budgets_cpu.py asserts element by element): it asks no less, and a bug of the size of
    the O rounding no longer hides behind it.
  * dV: sum_i Pe_ij |dO_id| plus one output ulp.
  * dQ, dK: with e_dP_ij = (hd + 1) u' sum_d |dO_id| |v_jd| and E_ij = |dS_ij| (ulp16 + e_p) + P_ij (e_delta_i + e_dP_ij) + floor:
    scale sum_j E_ij |k_jd| resp. scale sum_i E_ij |q_id|, plus one output ulp; the fp32 partial-dQ slices of T > 256 add
    nkt u |dQ|.
Every output ulp is taken at |reference| + the rest of the budget (gemm_ref._rounded).

RESTATEMENTS (restatement()): fp32 torch with .to(half).float() where the kernel rounds, in the order of the path family the cell
reaches: `onepass` (attn_fwd256p / 256v: max of the raw scores, p = exp2(fma(s, sc2, -m)), l from the fp32 p or (ONES) the rounded
ones, O = (P16 V) rcp(l)); `online` (attn_fwd_kernel: 64-key sub-blocks, the alpha rescale); `rows` (attn_fwd_rows_kernel for the
<= 16 tail rows: q pre-scaled, fp32 p, a division; the full blocks online); `tail` (attn_fwd_kernel<64, true>: the tail rows over
two 128-key halves per tile, each with its own online softmax, merged at the end); the backward (p = exp2(fma(s, sc2, -lse LOG2E)),
dS = p (dP - delta) in fp32, P and dS rounded before the dV / dK / dQ products, the scale after the accumulation; T > 256: one
fp32 dQ slice per 256-key tile, summed in tile order).  MUTATIONS are the realistic bugs of exactly this code; mutation_applies
says which (mutation, cell, T) can hold the bug at all.
"""
import math
from collections import namedtuple

import torch

from tests.rowpass_ref import DTYPE, U, ulp_out, worst

KINDS16 = ("bf16", "fp16")
MANT = {"bf16": 7, "fp16": 10}
LOG2E, LN2 = 1.4426950408889634, 0.6931471805599453
ITEM_LOOP = dict(bh=(9, 11), reserve=224)

Cell = namedtuple("Cell", "entry kernel hd cases bh reserve comm family cond")


def _cell(entry, kernel, hd, cases, family, cond, bh=(2, 3), reserve=0, comm=False):
    return Cell(entry, kernel, hd, tuple(cases), bh, reserve, comm, family, cond)


_LOOP = "99 items on 32 workgroups: three or four items each"
_P_T = ((1, "one key, one query"), (16, "one 16-row tile"), (17, "one row in the second tile"), (65, "one key in the second sub-block"),
        (100, "ragged second sub-block"), (255, "one key short of the full tile"))
_KS_T = ((1, "one key, one query: dQ = dK = 0"), (16, "one tile"), (100, "ragged second chunk"), (129, "one row in the third chunk"))
_LONG_T = ((272, "last key tile of 16 keys"), (320, "last key tile of 64"), (512, "two full tiles"), (784, "three full tiles + 16"))


def _cells():
    c = []
    for hd in (64, 72):
        c.append(_cell("fwd", f"attn_fwd256v_kernel<{hd}>", hd, [(256, "the training shape")], "onepass", "T == 256 && (hd == 64 || hd == 72)"))
        c.append(_cell("fwd", f"attn_fwd256v_kernel<{hd}>", hd, [(256, _LOOP)], "onepass", "T == 256 && (hd == 64 || hd == 72)", **ITEM_LOOP))
        c.append(_cell("fwd", f"attn_fwd256p_kernel<{hd}, false>", hd, _P_T, "onepass", "T < 256"))
        c.append(_cell("fwd", f"attn_fwd256p_kernel<{hd}, false>", hd, [(100, _LOOP)], "onepass", "T < 256", **ITEM_LOOP))
    c.append(_cell("fwd", "attn_fwd256p_kernel<80, *>", 80, [(77, "FULL = false; ragged second sub-block"), (256, "FULL = true")], "onepass",
                   "T <= 256 && hd == 80"))
    c.append(_cell("fwd", "attn_fwd_kernel<64>", 64, [(273, "one row too many for the row kernel"), (320, "a 64-row second block"),
                                                       (529, "three blocks, 17 rows in the last")], "online", "T > 256, tail == 0 || tail > 16"))
    c.append(_cell("fwd", "attn_fwd_kernel<72>", 72, [(257, "one row in the second block"), (300, "ragged second block"),
                                                       (1040, "five blocks, the last has 16 rows")], "online", "T > 256 && hd == 72"))
    c.append(_cell("fwd", "attn_fwd_rows_kernel + attn_fwd_kernel<64>", 64, [(257, "one tail row"), (261, "five tail rows"), (272, "16 tail rows")],
                   "rows", "hd == 64 && 256 < T <= 512 && 1 <= T % 256 <= 16"))
    c.append(_cell("fwd", "attn_fwd_kernel<64, true>", 64, [(513, "one tail row past two tiles"), (528, "16 tail rows"),
                                                             (1029, "five tail rows past four tiles"), (4112, "the limit of the branch")],
                   "tail", "hd == 64 && 512 < T <= 4112 && 1 <= T % 256 <= 16"))
    for hd in (64, 72):
        c.append(_cell("bwd", f"attn_bwd_ks_kernel<{hd}>", hd, _KS_T + ((256, "the full tile"),), "bwd", "ws == NULL (T <= 256)"))
        c.append(_cell("bwd_ws", f"attn_delta_kernel + attn_bwd_ksp_kernel<{hd}>", hd, _KS_T + ((255, "one key short of the ring kernel"),),
                       "bwd", "ws && T < 256"))
        c.append(_cell("bwd_ws", f"attn_delta_kernel + attn_bwd_ksp_kernel<{hd}>", hd, [(64, _LOOP)], "bwd", "ws && T < 256", **ITEM_LOOP))
        c.append(_cell("bwd_ws", f"attn_delta_kernel + attn_bwd_ksp_kernel<{hd}>", hd, [(64, _LOOP + "; four short lists per CU")], "bwd",
                       "ws && T < 256, reed_concurrent_comm()", comm=True, **ITEM_LOOP))
        c.append(_cell("bwd_ws", f"attn_delta_kernel + attn_bwd_ring_kernel<{hd}>", hd, [(256, "the training shape")], "bwd", "ws && T == 256"))
        c.append(_cell("bwd_ws", f"attn_delta_kernel + attn_bwd_ring_kernel<{hd}>", hd, [(256, _LOOP)], "bwd", "ws && T == 256", **ITEM_LOOP))
        c.append(_cell("bwd_ws", f"attn_delta_kernel + attn_bwd_long_kernel<{hd}> + attn_dq_reduce_kernel", hd,
                       _LONG_T + (((1040, "four full tiles + 16"),) if hd == 72 else ()), "bwd", "ws && 256 < T <= 4096 && T % 16 == 0"))
        c.append(_cell("bwd_dp", f"attn_delta_combine_kernel + ksp / ring / long <{hd}>", hd,
                       [(100, "attn_bwd_ksp_kernel"), (256, "attn_bwd_ring_kernel"), (320, "attn_bwd_long_kernel")], "bwd", "dpart != NULL"))
    return tuple(c)


CELLS = _cells()
CASES = tuple((ci, T) for ci, c in enumerate(CELLS) for T, _ in c.cases)


def bh_of(cell, T):
    """(B, H) of a case: the cell's, smaller where T is long (the fp64 reference holds T x T matrices per item)."""
    return (1, 1) if T > 2048 else (1, 2) if T > 600 else cell.bh


def cell_id(ci):
    c = CELLS[ci]
    k = c.kernel.split(" + ")[-2 if c.kernel.endswith("reduce_kernel") else -1].replace("attn_", "").replace("_kernel", "").replace(" ", "")
    return f"{c.entry}-{k}" + ("-hd%d" % c.hd if "<" not in k else "") + ("-loop" if c.reserve else "") + ("-comm" if c.comm else "")


def case_id(case):
    return f"{cell_id(case[0])}-T{case[1]}"


def flavours(cell, kind):
    f = ("unit", "peaked")
    return f + (("small_do", "big_do") if kind == "fp16" and cell.entry != "fwd" else ())


def ones_cell(cell, T):
    """The forward takes the softmax denominator from the ones column of V (attn_fwd256p / 256v, ONES = (HD == 72))."""
    return cell.entry == "fwd" and cell.hd == 72 and T <= 256


def ws_floats(B, T, H):
    """reed_attention_bwd_ws_floats restated (the GPU test asks the library)."""
    n = B * T * H
    return n if T <= 256 else n * (1 + -(-T // 256) * 72)


# ---------------------------------------------------------------------------------------------------------------- inputs
def _exact_fwd(q, k, v, hd, r0=0, r1=None):
    """fp64 S, m, l, lse, P, O of the query rows r0:r1."""
    S = (q[:, r0:r1] @ k.transpose(1, 2)) * hd ** -0.5
    m = S.max(-1).values
    l = torch.exp(S - m[..., None]).sum(-1)
    lse = m + torch.log(l)
    P = torch.exp(S - lse[..., None])
    return S, m, l, lse, P, P @ v


def inputs(ci, T, kind, flavour):
    """Everything the case's call reads, logical [B H, T, hd] in the build's type (lse, dpart fp32)."""
    cell = CELLS[ci]
    (B, H), hd, dt = bh_of(cell, T), cell.hd, DTYPE[kind]
    N = B * H
    g = torch.Generator().manual_seed(977 + 131 * ci + 7 * T + {"unit": 0, "peaked": 1, "small_do": 2, "big_do": 3}[flavour])
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    q, k, v, dO = rn(N, T, hd), rn(N, T, hd), rn(N, T, hd), rn(N, T, hd)
    k[..., 0] = k[..., 0].abs() + 1
    if flavour == "peaked":
        q, k = 2.5 * q, 2.5 * k
    dO = dO * {"small_do": 2.0 ** -14, "big_do": 2.0 ** 10}.get(flavour, 1.0)
    if T >= 8:
        q[:, 1] = 0
        k[:, 3] = k[:, 2]
        q[:, 4] *= 8
        q[:, 5] = 0
        q[:, 5, 0] = -64
        k = k.to(dt).double()
        q[:, T - 1] = 6 * k[:, T - 1]
    inp = dict(ci=ci, cell=cell, T=T, kind=kind, flavour=flavour, B=B, H=H, hd=hd, q=q.to(dt), k=k.to(dt), v=v.to(dt), dO=dO.to(dt))
    if cell.entry != "fwd":
        q64, k64, v64 = inp["q"].double(), inp["k"].double(), inp["v"].double()
        _, _, _, lse, _, O = _exact_fwd(q64, k64, v64, hd)
        inp["O"], inp["lse"] = O.to(dt), lse.float()
        if cell.entry == "bwd_dp":
            pr = (inp["dO"].double() * inp["O"].double()).view(B, H, T, hd)
            slots = [pr[..., :64].sum(-1)] + ([pr[..., 64:].sum(-1)] if hd > 64 else [])
            inp["dpart"] = torch.stack([s.permute(1, 0, 2).reshape(H, B * T) for s in slots], 1).float()     # [H, S, B T]
    return inp


# -------------------------------------------------------------------------------------------------------- fp64 reference
_RB = 1024      # query rows per block of the forward reference (T = 4112: 17 M scores per item)


def reference(inp, stated=False):
    """{output: (fp64 reference, budget)}: O, lse of a forward case; dQ, dK, dV of a backward one.  Logical [B H, T, hd] / [B H, T].
    stated: the backward with delta from the exact O and the O-rounding term in the budget (see the module docstring)."""
    cell, T, kind, hd = inp["cell"], inp["T"], inp["kind"], inp["hd"]
    q, k, v = inp["q"].double(), inp["k"].double(), inp["v"].double()
    n, up, u16, floor = T + hd + 8, 2 * U, 2.0 ** -MANT[kind], float(ulp_out(0.0, kind))
    scale = hd ** -0.5
    if cell.entry == "fwd":
        Os, bOs, ls, bls = [], [], [], []
        for r0 in range(0, T, _RB):
            S, m, l, lse, P, O = _exact_fwd(q, k, v, hd, r0, r0 + _RB)
            e_p = n * up * (1 + lse.abs()[..., None] + S.abs())
            Pe = P * (u16 + e_p) + floor * torch.exp(m - lse)[..., None]
            rest = Pe @ v.abs() + Pe.sum(-1, keepdim=True) * O.abs()
            bl = n * up * (1 + lse.abs() + S.abs().max(-1).values) + ulp_out(torch.log(l), "fp32")
            if ones_cell(cell, T):
                bl = bl + u16
            Os.append(O), bOs.append(_rounded(O, rest, kind)), ls.append(lse), bls.append(bl)
        return dict(O=(torch.cat(Os, 1), torch.cat(bOs, 1)), lse=(torch.cat(ls, 1), torch.cat(bls, 1)))
    dO, O16, lse32 = inp["dO"].double(), inp["O"].double(), inp["lse"].double()
    S, _, _, lse, P, O = _exact_fwd(q, k, v, hd)
    dP = dO @ v.transpose(1, 2)
    delta = (dO * (O if stated else O16)).sum(-1)
    dS = P * (dP - delta[..., None])
    dQ, dK, dV = scale * dS @ k, scale * dS.transpose(1, 2) @ q, P.transpose(1, 2) @ dO
    e_p = u16 + n * up * (1 + lse32.abs()[..., None] + S.abs())               # ulp16 + e_p of the docstring
    Pe = P * e_p + floor
    e_delta = (hd + 1) * up * (dO * O16).abs().sum(-1) + ((dO.abs() * (O16 - O).abs()).sum(-1) if stated else 0)
    e_dP = (hd + 1) * up * (dO.abs() @ v.abs().transpose(1, 2))
    E = dS.abs() * e_p + P * (e_delta[..., None] + e_dP) + floor
    rQ = scale * E @ k.abs() + (-(-T // 256) * U * dQ.abs() if T > 256 else 0)
    rK = scale * E.transpose(1, 2) @ q.abs()
    rV = Pe.transpose(1, 2) @ dO.abs()
    return dict(dQ=(dQ, _rounded(dQ, rQ, kind)), dK=(dK, _rounded(dK, rK, kind)), dV=(dV, _rounded(dV, rV, kind)))


def _rounded(ref, rest, kind):
    """Budget of an output rounded to the 16-bit type whose unrounded value is within `rest` of ref: the whole ulp is taken at
    |ref| + rest, the computed value being what is rounded (tests/gemm_ref.py)."""
    return rest + ulp_out(ref.abs() + rest, kind)


def ratios(got, ref):
    """{output: (worst error / budget, flat index)}; every element counts."""
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    return {k: worst((got[k].double().flatten() - ref[k][0].flatten()).abs(), ref[k][1].flatten()) for k in ref}


def decode(inp, name, flat):
    """Flat index of a logical output -> (b, h, t, d) (d = None for lse)."""
    T, hd, H = inp["T"], inp["hd"], inp["H"]
    if name == "lse":
        return flat // (H * T), flat // T % H, flat % T, None
    return flat // (H * T * hd), flat // (T * hd) % H, flat // hd % T, flat % hd


# -------------------------------------------------------------------------------------------------------- fp32 restatement
MUTATIONS = ("scale_of_hd64", "keys_not_masked", "last_key_dropped", "last_query_dropped", "cols_from_64_not_stored", "lse_base2",
             "lse_without_m", "delta_omitted", "delta_of_next_head", "delta_of_next_row", "delta_slot0_only", "dk_without_scale",
             "last_dq_slice_not_reduced", "stale_row_of_previous_item", "alpha_skipped_on_last_tile")


def mutation_applies(m, cell, T):
    """Whether mutation m is a bug this (cell, T) can have at all: the code it breaks runs here."""
    fwd = cell.entry == "fwd"
    B, H = bh_of(cell, T)
    if m == "scale_of_hd64":                            # rsqrtf((float)HD) with the wrong HD
        return cell.hd != 64
    if m == "keys_not_masked":                          # the forward's -inf select of a ragged sub-block (the backward's phantom
        return fwd and T % 64 != 0                      # keys meet zero K rows: nothing to get wrong)
    if m in ("last_key_dropped", "last_query_dropped"):
        return T >= 2
    if m == "cols_from_64_not_stored":
        return cell.hd != 64
    if m in ("lse_base2", "lse_without_m"):
        return fwd
    if m == "delta_omitted":
        return not fwd
    if m == "delta_of_next_head":
        return not fwd and H >= 2
    if m == "delta_of_next_row":
        return not fwd and T >= 2
    if m == "delta_slot0_only":
        return cell.entry == "bwd_dp" and cell.hd == 72
    if m == "dk_without_scale":
        return not fwd
    if m == "last_dq_slice_not_reduced":
        return not fwd and T > 256
    if m == "stale_row_of_previous_item":               # a V row of the forward / a K row of the dQ product from item n - 1
        return B * H >= 2
    if m == "alpha_skipped_on_last_tile":               # where the one-hot last row walks the online loop
        return cell.family in ("online", "tail")
    raise ValueError(m)


def _c32(x):
    return torch.tensor(x, dtype=torch.float32)


def _exp2_fma(s, sc2, sub):
    """exp2(fma(s, sc2, -sub)) in fp32: the product and the difference rounded once."""
    return torch.exp2((s.double() * float(sc2) - sub.double()).float())


def _online(q, ranges, k, v, sc2, r, skip_alpha_last=False):
    """attn_fwd_kernel's online softmax over the key ranges in order: (m, l, unnormalised O), m in the log2 domain."""
    N, R, hd = q.shape
    m, l, o = torch.full((N, R), -math.inf), torch.zeros(N, R), torch.zeros(N, R, hd)
    for n_, (k0, k1) in enumerate(ranges):
        s = q @ k[:, k0:k1].transpose(1, 2)
        mnew = torch.maximum(m, s.max(-1).values * sc2)
        alpha = torch.exp2(m - mnew)
        p = _exp2_fma(s, sc2, mnew[..., None])
        l = l * alpha + p.sum(-1)
        if not (skip_alpha_last and n_ == len(ranges) - 1):
            o = o * alpha[..., None]
        o = o + r(p) @ v[:, k0:k1]
        m = mnew
    return m, l, o


def _prev_item_row(x, row):
    """x [N, T, hd] with row `row` of every item but the first taken from the item before it."""
    x = x.clone()
    x[1:, row] = x[:-1, row].clone()
    return x


def restatement(inp, mutation=None):
    """The kernels' own order of operations in fp32 torch -> the logical outputs (float tensors)."""
    assert mutation is None or mutation in MUTATIONS
    cell, T, kind, hd, B, H = inp["cell"], inp["T"], inp["kind"], inp["hd"], inp["B"], inp["H"]
    dt = DTYPE[kind]
    r = lambda x: x.to(dt).float()  # noqa: E731
    q, k, v = inp["q"].float(), inp["k"].float(), inp["v"].float()
    N = B * H
    sc = torch.rsqrt(_c32(64.0 if mutation == "scale_of_hd64" else float(hd)))
    sc2 = sc * _c32(LOG2E)
    if cell.entry == "fwd":
        Tk = T
        if mutation == "keys_not_masked":               # a whole 16-key tile of zero rows behind the last key, scores 0
            k, v, Tk = torch.cat([k, torch.zeros(N, 16, hd)], 1), torch.cat([v, torch.zeros(N, 16, hd)], 1), T + 16
        if mutation == "last_key_dropped":
            k, v, Tk = k[:, :T - 1], v[:, :T - 1], T - 1
        if mutation == "stale_row_of_previous_item":
            v = _prev_item_row(v, Tk - 1)
        skip = mutation == "alpha_skipped_on_last_tile"
        if cell.family == "onepass":
            s = q @ k.transpose(1, 2)
            mneg = s.max(-1).values * sc2
            p = _exp2_fma(s, sc2, mneg[..., None])
            p16 = r(p)
            l = (p16 if ones_cell(cell, T) else p).sum(-1)
            O = r((p16 @ v) * (1.0 / l)[..., None])
            m2, ll = mneg, l
        else:
            main = T if cell.family == "online" else T - T % 256
            m2, ll, o = _online(q[:, :main], [(k0, min(k0 + 64, Tk)) for k0 in range(0, Tk, 64)], k, v, sc2, r, skip)
            O = r(o * (1.0 / ll)[..., None])
            if cell.family == "rows":                   # one wave per row: q pre-scaled, fp32 p, exact division
                s = (q[:, main:] * sc) @ k.transpose(1, 2)
                mx = s.max(-1).values
                p = torch.exp2((s - mx[..., None]) * _c32(LOG2E))
                sm = p.sum(-1)
                O = torch.cat([O, r((p @ v) / sm[..., None])], 1)
                m2, ll = torch.cat([m2, mx * _c32(LOG2E)], 1), torch.cat([ll, sm], 1)
            if cell.family == "tail":                   # two 128-key halves per tile, merged in a fixed order
                tiles = range(0, Tk, 256)
                h0 = [(k0, min(k0 + 128, Tk)) for k0 in tiles]
                h1 = [(k0 + 128, min(k0 + 256, Tk)) for k0 in tiles if k0 + 128 < Tk]
                (m0, l0, o0), (m1, l1, o1) = _online(q[:, main:], h0, k, v, sc2, r, skip), _online(q[:, main:], h1, k, v, sc2, r, skip)
                mm = torch.maximum(m0, m1)
                a0, a1 = torch.exp2(m0 - mm), torch.exp2(m1 - mm)
                lt = l0 * a0 + l1 * a1
                O = torch.cat([O, r((o0 * a0[..., None] + o1 * a1[..., None]) * (1.0 / lt)[..., None])], 1)
                m2, ll = torch.cat([m2, mm], 1), torch.cat([ll, lt], 1)
        lse = m2 * _c32(LN2) + torch.log(ll)
        if mutation == "lse_base2":
            lse = m2 + torch.log2(ll)
        if mutation == "lse_without_m":
            lse = torch.log(ll)
        if mutation == "last_query_dropped":            # never written: the NaN fill stays
            O, lse = O.clone(), lse.clone()
            O[:, T - 1], lse[:, T - 1] = math.nan, math.nan
        if mutation == "cols_from_64_not_stored":
            O = O.clone()
            O[..., 64:] = 0
        return dict(O=O, lse=lse)
    dO = inp["dO"].float()
    if cell.entry == "bwd_dp":
        dpart = inp["dpart"]
        delta = dpart[:, 0] + dpart[:, 1] if dpart.shape[1] == 2 and mutation != "delta_slot0_only" else dpart[:, 0]
        delta = delta.view(H, B, T).permute(1, 0, 2).reshape(N, T)
    else:
        delta = (dO * inp["O"].float()).sum(-1)
    if mutation == "delta_omitted":
        delta = torch.zeros_like(delta)
    if mutation == "delta_of_next_head":
        delta = delta.view(B, H, T).roll(-1, 1).reshape(N, T)
    if mutation == "delta_of_next_row":
        delta = delta.roll(-1, 1)
    p = _exp2_fma(q @ k.transpose(1, 2), sc2, (inp["lse"] * _c32(LOG2E))[..., None])
    ds = p * (dO @ v.transpose(1, 2) - delta[..., None])
    p16, ds16 = r(p), r(ds)
    p16k, ds16k = p16, ds16                              # what the dV / dK products see
    if mutation == "last_query_dropped":
        p16k, ds16k = p16.clone(), ds16.clone()
        p16k[:, T - 1], ds16k[:, T - 1] = 0, 0
    dV = r(p16k.transpose(1, 2) @ dO)
    dK = r((ds16k.transpose(1, 2) @ q) * (1.0 if mutation == "dk_without_scale" else sc))
    kq = _prev_item_row(k, T // 2) if mutation == "stale_row_of_previous_item" else k
    if mutation == "last_key_dropped":
        ds16 = ds16.clone()
        ds16[..., T - 1] = 0
    if T <= 256:
        dQ = r((ds16 @ kq) * sc)
    else:
        tiles = [(k0, min(k0 + 256, T)) for k0 in range(0, T, 256)]
        if mutation == "last_dq_slice_not_reduced":
            tiles = tiles[:-1]
        dQ = torch.zeros(N, T, hd)
        for k0, k1 in tiles:
            dQ = dQ + (ds16[..., k0:k1] @ kq[:, k0:k1]) * sc
        dQ = r(dQ)
    out = dict(dQ=dQ, dK=dK, dV=dV)
    if mutation == "cols_from_64_not_stored":
        for t in out.values():
            t[..., 64:] = 0
    return out


# ------------------------------------------------------------------------------------------------------- guarded buffers
class Band:
    """A buffer of `shape` as a slice of a larger NaN allocation: guard elements (two rows of the buffer at least, a multiple of 64
    so that the slice keeps 16-byte alignment) in front and behind.  vals: what the live part holds; None leaves it NaN (an output)."""

    def __init__(self, shape, dtype, vals=None, device="cpu"):
        self.shape, self.n = tuple(shape), math.prod(shape)
        self.guard = -(-2 * max(math.prod(shape[1:]), 1) // 64) * 64
        self.full = torch.full((self.n + 2 * self.guard,), math.nan, dtype=dtype, device=device)
        self.live = self.full[self.guard:self.guard + self.n].view(self.shape)
        if vals is not None:
            self.live.copy_(vals.reshape(self.shape))

    def check(self, what, finite=True):
        """Every guard element still NaN; every live element finite (finite = False: a scratch buffer, guards only)."""
        f = self.full.detach().cpu().float()
        lo, hi = f[:self.guard], f[self.guard + self.n:]
        assert torch.isnan(lo).all(), f"{what}: written in front of the buffer at {int((~torch.isnan(lo)).nonzero()[0]) - self.guard}"
        assert torch.isnan(hi).all(), f"{what}: written behind the buffer at + {int((~torch.isnan(hi)).nonzero()[0])}"
        if finite:
            bad = ~torch.isfinite(f[self.guard:self.guard + self.n])
            assert not bad.any(), (f"{what}: {int(bad.sum())} live elements not finite (never written, or a NaN read from a guard), "
                                   f"first at {int(bad.nonzero()[0])}")
        return self


def to_qkv(inp, q, k, v):
    """Logical [B H, T, hd] x 3 -> the physical [B, T, 3, H, hd]."""
    B, H, T, hd = inp["B"], inp["H"], inp["T"], inp["hd"]
    return torch.stack([x.reshape(B, H, T, hd).permute(0, 2, 1, 3) for x in (q, k, v)], 2)


def to_rows(inp, x):
    """Logical [B H, T, hd] -> the physical [B, T, H hd] of O and dO."""
    B, H, T, hd = inp["B"], inp["H"], inp["T"], inp["hd"]
    return x.reshape(B, H, T, hd).permute(0, 2, 1, 3).reshape(B, T, H * hd)


def from_rows(inp, x):
    B, H, T, hd = inp["B"], inp["H"], inp["T"], inp["hd"]
    return x.reshape(B, T, H, hd).permute(0, 2, 1, 3).reshape(B * H, T, hd)


def from_qkv(inp, x):
    B, H, T, hd = inp["B"], inp["H"], inp["T"], inp["hd"]
    return [t.reshape(B * H, T, hd) for t in x.reshape(B, T, 3, H, hd).permute(2, 0, 3, 1, 4).unbind(0)]


def buffers(inp, device="cpu"):
    """Every buffer of the case's call as a Band: inputs filled, outputs NaN.  ws is sized by the caller (the library's count)."""
    cell, kind, B, H, T, hd = inp["cell"], inp["kind"], inp["B"], inp["H"], inp["T"], inp["hd"]
    dt, f32 = DTYPE[kind], torch.float32
    b = dict(qkv=Band((B, T, 3, H, hd), dt, to_qkv(inp, inp["q"], inp["k"], inp["v"]), device))
    if cell.entry == "fwd":
        b["o"], b["lse"] = Band((B, T, H * hd), dt, None, device), Band((B, H, T), f32, None, device)
        return b
    b["do"] = Band((B, T, H * hd), dt, to_rows(inp, inp["dO"]), device)
    b["lse"] = Band((B, H, T), f32, inp["lse"], device)
    b["dqkv"] = Band((B, T, 3, H, hd), dt, None, device)
    if cell.entry == "bwd_dp":
        b["dpart"] = Band(tuple(inp["dpart"].shape), f32, inp["dpart"], device)
    else:
        b["o"] = Band((B, T, H * hd), dt, to_rows(inp, inp["O"]), device)
    return b


OUTPUTS = {"fwd": ("o", "lse"), "bwd": ("dqkv",), "bwd_ws": ("dqkv",), "bwd_dp": ("dqkv",)}


def store(inp, bufs, out):
    """The logical outputs of a restatement written into the case's output Bands as a kernel would."""
    dt = DTYPE[inp["kind"]]
    if inp["cell"].entry == "fwd":
        bufs["o"].live.copy_(to_rows(inp, out["O"]).to(dt))
        bufs["lse"].live.copy_(out["lse"].reshape(bufs["lse"].shape))
    else:
        bufs["dqkv"].live.copy_(to_qkv(inp, out["dQ"], out["dK"], out["dV"]).to(dt))


def collect(inp, bufs):
    """Guards and finiteness of every buffer of the call checked (inputs: guards; outputs: both) -> the logical outputs (CPU)."""
    outs = OUTPUTS[inp["cell"].entry]
    for name, band in bufs.items():
        band.check(name, finite=name in outs)
    if inp["cell"].entry == "fwd":
        return dict(O=from_rows(inp, bufs["o"].live.cpu()), lse=bufs["lse"].live.cpu().reshape(-1, inp["T"]))
    dq, dk, dv = from_qkv(inp, bufs["dqkv"].live.cpu())
    return dict(dQ=dq, dK=dk, dV=dv)
