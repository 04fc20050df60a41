"""The 16-bit attention backward past 256 tokens (512^2 training: T = 1024) against a plain PyTorch fp32 softmax(q k^T / sqrt(hd)) v on
the same 16-bit q, k, v, in the bf16 and fp16 builds: csrc/attention.hip:attn_bwd_long_kernel (item = batch, head, 256-key tile) and
attn_dq_reduce_kernel (the fp32 partial-dQ slices summed in tile order) behind reed_attention_bwd_ws / reed_attention_bwd_dp."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _ref(qkv, B, T, H, hd):
    q, k, v = qkv.float().reshape(B, T, 3, H, hd).permute(2, 0, 3, 1, 4).unbind(0)
    s = (q @ k.transpose(-1, -2)) * hd ** -0.5
    p = s.softmax(-1)
    return (p @ v).transpose(1, 2).reshape(B, T, H * hd)


def _inputs(dev, B, T, H, hd, hdt, seed):
    from reed_amd import ops
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, T, 3, H, hd, generator=g).to(hdt).to(dev)
    do = torch.randn(B, T, H * hd, generator=g).to(hdt).to(dev)
    o = torch.zeros(B, T, H * hd, dtype=hdt, device=dev)
    lse = torch.zeros(B, H, T, device=dev)
    ops.attention_fwd(qkv, o, lse, B, T, H, hd)
    return qkv, do, o, lse


@pytest.fixture(params=["bf16", "fp16"])
def prec(request):
    from reed_amd import ops
    prev = ops.use(request.param)
    yield request.param
    ops.use(prev)


# (1, 320, 3, 64): a last key tile of 64 keys (waves without a key) and a last query chunk of 0 rows past 256 + 64; (2, 576, 6, 64):
# 384^2, a last key tile of 64 and a last query chunk of 0; (1, 4096, 2, 64): 16 key tiles and 64 chunks; (32, 1024, 16, 72): SiT-XL/2
# at 512^2, 2048 items, several per workgroup
@pytest.mark.parametrize("B,T,H,hd", [(1, 320, 3, 64), (2, 512, 4, 72), (2, 576, 6, 64), (1, 1024, 2, 72), (3, 1024, 16, 72),
                                       (1, 4096, 2, 64), (32, 1024, 16, 72)])
def test_attention_bwd_long(dev, prec, B, T, H, hd):
    from reed_amd import ops
    hdt = ops.half_dtype(prec)
    qkv, do, o, lse = _inputs(dev, B, T, H, hd, hdt, 5 + T)
    dqkv = torch.full_like(qkv, float("nan"))
    ws = torch.full((ops.attention_bwd_ws_floats(B, T, H),), float("nan"), device=dev)
    ops.attention_bwd(qkv, o, do, lse, dqkv, B, T, H, hd, ws=ws)
    q32 = qkv.float().requires_grad_(True)
    _ref(q32, B, T, H, hd).backward(do.float())
    ref = q32.grad
    nf = ~torch.isfinite(dqkv.float())
    assert not nf.any(), (int(nf.sum()), nf.nonzero()[:6].tolist())
    for w, name in enumerate("qkv"):
        a, r = dqkv[:, :, w].float(), ref[:, :, w]
        err = (a - r).abs().max().item()
        assert err <= 3e-2 * max(1.0, r.abs().max().item()), (name, err, r.abs().max().item())
        cos = torch.nn.functional.cosine_similarity(a.flatten(), r.flatten(), dim=0).item()
        assert cos > 0.9995, (name, cos)


@pytest.mark.parametrize("B,T,H,hd", [(32, 1024, 16, 72), (5, 576, 12, 64)])
def test_attention_bwd_long_bits_whatever_the_grid(dev, B, T, H, hd):
    """Twice -> identical bits; with set_concurrent_comm(True) (4 x the grid) and with CU reserves 32 / 200 (smaller grids) the items
    are the same and independent: identical bits again."""
    from reed_amd import ops
    ops.set_comm_forms(True)
    qkv, do, o, lse = _inputs(dev, B, T, H, hd, torch.bfloat16, B + T)
    ws = torch.empty(ops.attention_bwd_ws_floats(B, T, H), device=dev)
    outs = []
    for comm, reserve in ((False, 0), (False, 0), (True, 0), (False, 32), (False, 200)):
        dqkv = torch.full_like(qkv, float("nan"))
        ops.set_concurrent_comm(comm)
        ops.set_cu_reserve(reserve)
        try:
            ops.attention_bwd(qkv, o, do, lse, dqkv, B, T, H, hd, ws=ws)
        finally:
            ops.set_concurrent_comm(False)
            ops.set_cu_reserve(0)
        torch.cuda.synchronize()
        outs.append(dqkv)
    assert torch.isfinite(outs[0].float()).all()
    for x in outs[1:]:
        assert torch.equal(outs[0], x)


@pytest.mark.parametrize("b,H,hd,force", [(16, 16, 72, 258), (16, 6, 64, 0)])
def test_attention_bwd_long_delta_from_the_dgrad_epilogue(dev, prec, b, H, hd, force):
    """T = 1024: reed_gemm epilogue 13 + reed_attention_bwd_dp (delta from the partial dot products, O not read) equals the
    workspace form to 16-bit resolution, and twice -> identical bits (same token count and width as the T = 256 cases of
    test_attention_gpu.py::test_delta_from_the_dgrad_epilogue)."""
    from reed_amd import ops
    T = 1024
    D, M = H * hd, b * T
    hdt = ops.half_dtype(prec)
    g = torch.Generator().manual_seed(b + hd)
    dy = (torch.randn(M, D, generator=g) * 0.5).to(hdt).to(dev)
    w = (torch.randn(D, D, generator=g) / D ** 0.5).to(hdt).to(dev)
    qkv = torch.randn(b, T, 3, H, hd, generator=g).to(hdt).to(dev)
    with ops.forced_tile(force):
        o = torch.zeros(b, T, D, dtype=hdt, device=dev)
        lse = torch.zeros(b, H, T, device=dev)
        ops.attention_fwd(qkv, o, lse, b, T, H, hd)
        do0 = torch.empty(M, D, dtype=hdt, device=dev)
        ops.gemm(ops.NN, ops.EPI_BF16, dy, w, M, D, D, do0, D, D, D)
        S = 1 if hd == 64 else 2
        runs = []
        for _ in range(2):
            do1 = torch.full((M, D), float("nan"), dtype=hdt, device=dev)
            dpart = torch.full((H, S, M), float("nan"), device=dev)
            assert ops.dgrad_with_head_dots(dy, w, do1, o, dpart, M, D, D, hd)
            dq = torch.full_like(qkv, float("nan"))
            ws = torch.full((ops.attention_bwd_ws_floats(b, T, H),), float("nan"), device=dev)
            ops.attention_bwd_dp(qkv, do1, lse, dpart, dq, ws, b, T, H, hd)
            torch.cuda.synchronize()
            runs.append((do1, dpart, dq))
        assert all(torch.equal(x, y) for x, y in zip(runs[0], runs[1]))
        dq = runs[0][2]
        dq0 = torch.full_like(qkv, float("nan"))
        ops.attention_bwd(qkv, o, do0, lse, dq0, b, T, H, hd, ws=torch.empty_like(ws))
        a, r = dq.float(), dq0.float()
        assert torch.isfinite(a).all() and (a - r).abs().max().item() <= 1e-2 * r.abs().max().item()


def test_attention_bwd_long_refusals(dev):
    """T = 1000 (not a multiple of 16), T = 4112 (past 4096) and T > 256 on the workspace-free entry are refused by the ABI with a
    message; nothing is launched (dqkv keeps its NaNs)."""
    from reed_amd import ops
    for T, with_ws, what in ((1000, True, "multiple of 16"), (4112, True, "4096"), (512, False, "reed_attention_bwd_ws")):
        B, H, hd = 1, 2, 72
        qkv, do, o, lse = _inputs(dev, B, T, H, hd, torch.bfloat16, T)
        dqkv = torch.full_like(qkv, float("nan"))
        ws = torch.empty(ops.attention_bwd_ws_floats(B, T, H), device=dev) if with_ws else None
        with pytest.raises(RuntimeError, match=what):
            ops.attention_bwd(qkv, o, do, lse, dqkv, B, T, H, hd, ws=ws)
        torch.cuda.synchronize()
        assert torch.isnan(dqkv.float()).all()


def test_attention_bwd_ws_floats(dev):
    """T <= 256: B T H (delta only), pinned; T > 256: delta + ceil(T / 256) partial-dQ slices sized for hd 72."""
    from reed_amd import ops
    for prec in ("bf16", "fp16"):
        prev = ops.use(prec)
        try:
            for B, T, H in ((1, 16, 2), (128, 256, 16), (3, 200, 5), (40, 128, 16)):
                assert ops.attention_bwd_ws_floats(B, T, H) == B * T * H
            for B, T, H in ((32, 1024, 16), (1, 320, 3), (2, 4096, 2)):
                assert ops.attention_bwd_ws_floats(B, T, H) == B * T * H * (1 + -(-T // 256) * 72)
        finally:
            ops.use(prev)
