"""Forward / backward of the SiT model as a sequence of HIP kernel launches (reference: image/models/sit.py:271-311
and its autograd). Python here is orchestration only: shapes, pointers into the arenas, launch order, the
activation tape. Numerics follow the reference under accelerate bf16 mixed precision (SURVEY.md §3.2 dtype map):
fp32 residual stream / LayerNorm / loss, bf16 GEMM operands with fp32 MFMA accumulation, bf16 linear outputs.

Per block the launch sequence is
  fwd : LN+modulate -> qkv GEMM(+bias) -> attention -> proj GEMM(+bias, gate, residual) -> LN+modulate
        -> fc1 GEMM(+bias, GELU) -> fc2 GEMM(+bias, gate, residual)                       (7 launches)
  bwd : gate-bwd, 2x{wgrad, dgrad} for the MLP, LN-bwd, gate-bwd, proj {wgrad, dgrad}, attention-bwd,
        qkv {wgrad, dgrad}, LN-bwd, modulation-grad reduce                                (14 launches)
and the modulation of ALL blocks is one GEMM forward (silu(c) @ W_ada_all^T) and two backward.

Each decision has one site: a block linear's forward launch (16-bit or MX-fp8) is `linear` in Engine._forward, its parameter
gradients (grouped launch / own launch / adapters, as freeze.py's plan says) are Engine._lin_grads.  The backward runs as phases
over one per-call record: _backward_final, _backward_block for each block from the top, _backward_tail (adaLN + conditioning),
_backward_end (the buckets not yet fired, the inputs' gradients, the side stream's join) — full and truncated alike.
With SiT.recompute set (recompute.py) the lowest blocks keep a checkpoint (x, y2) in place of their record and _backward_block
starts by rebuilding it (_recompute_block: the forward's launches up to fc1); everything behind that reads the record as ever.
"""
import contextlib
import logging
import os
import types

import torch

from . import ops
from .freeze import LINEARS, FreezePlan
from .recompute import max_tokens, recomputed_blocks, saved_activation_bytes
from .ops import (NT, NN, TN, EPI_BF16, EPI_GELU, EPI_SILU, EPI_GATE_RES, EPI_DGELU, EPI_DSILU, EPI_F32, EPI_ADDF32_RB,
                  EPI_GELU_G, EPI_SILU_G, EPI_MUL)

logger = logging.getLogger(__name__)


def _allocators(hdt, dev):
    """(bf, f32): uninitialised arrays on `dev`, of the build's operand type `hdt` / of fp32."""
    def bf(*s):
        return torch.empty(s, dtype=hdt, device=dev)

    def f32(*s):
        return torch.empty(s, dtype=torch.float32, device=dev)

    return bf, f32


class Engine:
    # Kernel forms picked by the token count per GPU (both measured on MI355X with SiT-XL/2; bench.py prints them under
    # "kernel_forms", train.py logs them): the activation backward as one multiply by a derivative the forward saved — above this
    # many tokens (b > 48), see save_act_grad below — and the block's weight gradients on a second stream — up to this many.
    # NOTE for comparisons across GPU counts: the two activation-backward forms differ by one bf16 rounding of the derivative, so
    # 1 GPU x 256 and 8 GPUs x 32 of the same global batch do not give the same gradient bits unless the form is pinned
    # (train.py --save-act-grad {auto,0,1}; bench.py --save-act-grad).
    # (Round 6) the blocks' input gradients as NT GEMMs on a transposed copy of the weights from this many tokens per GPU on
    # (None: never): + 0.9 GB, kept fresh by the fused optimiser on its side stream; 3.6-5 % per dgrad GEMM at b = 256
    DGRAD_NT_MIN_TOKENS = 12289
    SAVE_ACT_GRAD_MIN_TOKENS = 12288
    # (Round 6: 0 = never by default.  With the one-item-per-CU weight-gradient launch the second stream measures equal at b = 32 —
    # 957.1 / 965.8 images/s with it, 963.7 / 958.4 without (profiles/r6_b32_side_stream_choices.txt) — and on the timeline it only
    # parks the main queue's row kernels behind a launch that holds every CU (ln_mod_bwd2: 131 us per launch for 30 us of work).
    # REED_WGRAD_STREAM=1 / engine.wgrad_stream = True switch it on; rounds 2-5 used it up to 12288 tokens: + 3.7 % at b = 32 with
    # the kernels of that time.)
    WGRAD_STREAM_MAX_TOKENS = 0

    def __init__(self, model):
        self.m = model
        self.L = model._layout
        self.A = model._arena
        if self.A.master.device.type != "cuda":
            raise RuntimeError("reed_amd.SiT: parameters are on %s; move the model to an AMD GPU (model.cuda()). "
                               "The hot path has no CPU fallback." % self.A.master.device)
        self.D = model.hidden_size
        self.H = model.num_heads
        self.hd = self.D // self.H
        self.Hm = int(self.D * model.mlp_ratio)
        self.T = model.num_patches
        self.P = model.patch_size
        self.C = model.in_channels
        self.depth = model.depth
        self.NO = self.P * self.P * self.C
        self._dims_ok = set()    # precisions whose shape restrictions this model has passed (_check_dims)
        split = model.encoder_depth_text is not None and model.encoder_depth_text != model.encoder_depth
        self.split = split
        self.tap_depth = [model.encoder_depth if (zt == "i" or not split) else model.encoder_depth_text
                          for zt in model.z_types]
        self.reducer = None      # set by reed_amd.parallel.GradReducer
        self._dot_delta = {}     # (tokens, operand type, reducing, forced tile, CU reserve, comm forms, NT dgrad) -> the dO GEMM has the head-dot epilogue
        self._ws = None
        self._named = None       # [(name, parameter)], cached: named_parameters() walks the module tree
        self._plans = {}         # (requires_grad signature, x needs grad, t needs grad) -> FreezePlan
        self._ws_side = None
        self._shadow_t = None
        self.dgrad_nt = None     # True / False / None = by DGRAD_NT_MIN_TOKENS: the blocks' dgrads as NT GEMMs on transposed weights
        self.split_ada_wgrad = None   # None: per-block adaLN weight gradients iff a reducer is attached (see backward)
        self._side = None        # second HIP stream: the blocks' weight-gradient GEMMs run beside the dgrad chain
        # True / False / None = by WGRAD_STREAM_MAX_TOKENS (above)
        self.wgrad_stream = {"0": False, "1": True}.get(os.environ.get("REED_WGRAD_STREAM", "auto"))
        self.wgrad_stream_max_tokens = self.WGRAD_STREAM_MAX_TOKENS
        self.grad_live = False   # True: param grads hold a previous micro-step -> accumulate
        self.table_rows = model.num_classes + (1 if model.class_dropout_prob > 0 else 0)
        self._hb = 2             # bytes per element of the current build's operand arrays (set per forward / backward)
        # Round 5: the forward epilogues of fc1 / the t-MLP / the projector layers save the activation's DERIVATIVE at the
        # pre-activation (in the array that used to hold the pre-activation: nothing but the backward's dGELU / dSiLU epilogue
        # read it), so that backward epilogue is one multiply per element.  False: the pre-activation and the recomputing
        # epilogues (the form the round-1..4 records were measured with; tests compare the two).
        # (same-box A/B at b = 256: dgrad fc2 0.729 -> 0.659 ms, fc1 forward 0.681 -> 0.708, step 199.1 -> 197.5 ms: profiles/r5_actgrad.txt)
        # None = by the token count: on above 12288 tokens (b > 48 per GPU), where the block's GEMMs run on the four-wave 256^2
        # kernels — one wave per SIMD, the dGELU epilogue's vector work exposed.  Below, the 256x144 kernel's two waves per SIMD
        # hide that work already and the derivative only costs the forward: b = 32, in-step, fc1 forward 123.8 -> 136.5 us per launch
        # against 118.1 -> 116.4 for the fc2 dgrad (profiles/r4_b32_timeline.txt, r5_b32_timeline_first.txt).
        self.save_act_grad = None
        # the attention backward's delta = rowsum(dO * O) from the epilogue of the GEMM that produces dO (False: the row kernel;
        # tests/test_model_gpu.py::test_bench_plan_matches_the_golden_pinned_plan_at_b256 compares the two)
        self.fused_delta = True
        self._fp8_logged = False  # the list of fp8 / 16-bit layers has been logged
        self._err = None         # sticky device flag: a label outside the embedding table was seen (see check_errors)
        self.recomputed = 0      # blocks the last backward rebuilt from their checkpoints (SiT.recompute; recompute.py)

    def _check_dims(self, prec):
        """Shape restrictions of the build that evaluates the model: the 16-bit MFMA tiles want every GEMM width in multiples
        of 128; the fp32-operand build (csrc/gemm_f32.hip) guards every bound and only needs 4-element alignment."""
        if prec in self._dims_ok:
            return
        q = 4 if prec == "fp32" else 128
        what = "4 (fp32 operands)" if prec == "fp32" else "128 for the MFMA GEMM tiles"
        for n, v in (("hidden_size", self.D), ("mlp hidden", self.Hm), ("projector_dim", self.m.projector_dim)):
            if v % q:
                raise ValueError(f"{n}={v} must be a multiple of {what}")
        for z in self.m.z_dims:
            if z % q:
                raise ValueError(f"z_dim={z} must be a multiple of {what}")
        self._dims_ok.add(prec)

    def check_errors(self):
        """Raise if any forward since the last check saw a class label outside the embedding table (the reference's
        nn.Embedding raises IndexError at that forward, sit.py:98; here the kernel substitutes row 0, sets a device flag
        and the error surfaces at the caller's next synchronisation point: the trainer's logging sync, the samplers'
        return, state_dict()). Costs one 4-byte D2H copy — call it where the host synchronises anyway."""
        if self._err is not None and int(self._err.item()) != 0:
            self._err.zero_()
            raise IndexError(f"reed_amd.SiT: a class label outside [0, {self.table_rows}) was passed to the model "
                             f"(num_classes={self.m.num_classes}, class_dropout_prob={self.m.class_dropout_prob}); "
                             "the affected forwards used row 0 instead")

    # ---- pointers into the arenas -------------------------------------------------
    def W(self, name):
        return self._shadow.data_ptr() + self._hb * self.L.off(name)

    def Wf(self, name):
        return self.A.master.data_ptr() + 4 * self.L.off(name)

    def G(self, name):
        return self.A.grad.data_ptr() + 4 * self.L.off(name)

    def ws(self, nfloats, dev):
        if self._ws is None or self._ws.numel() < nfloats:
            self._ws = torch.empty(int(nfloats), dtype=torch.float32, device=dev)
        return self._ws

    def ws_side(self, nfloats, dev):
        """Split-K slab workspace of the weight-gradient stream (allocated while that stream is current)."""
        if self._ws_side is None or self._ws_side.numel() < nfloats:
            self._ws_side = torch.empty(int(nfloats), dtype=torch.float32, device=dev)
        return self._ws_side

    # ---- forward -------------------------------------------------------------------
    FP8_LAYERS = LINEARS[::-1]   # the block linears in forward order

    def fp8_layers(self, tokens=None, precision=None):
        """{block linear: True where it runs on the MX-fp8 GEMM with SiT.fp8 set, False where it stays 16-bit} for a forward of
        `tokens` rows (default: one sample) — what reed_gemm_mxfp8_plan says of each layer's (epilogue, M, N, K), host arithmetic."""
        D, Hm = self.D, self.Hm
        M = int(tokens) if tokens else self.T
        prec = precision or self.m.precision
        if prec not in ("bf16", "fp16"):
            return {n: False for n in self.FP8_LAYERS}
        shapes = {"attn.qkv": (EPI_BF16, 3 * D, D), "attn.proj": (EPI_GATE_RES, D, D), "mlp.fc1": (EPI_GELU, Hm, D),
                  "mlp.fc2": (EPI_GATE_RES, D, Hm)}
        return {n: ops.gemm_mxfp8_plan(e, M, N, K, precision=prec) for n, (e, N, K) in shapes.items()}

    def max_tokens(self, precision=None):
        """The largest B T of a forward whose backward writes parameter gradients (recompute.max_tokens: the 32-bit byte offsets
        of the 16-bit weight-gradient GEMMs over their token-major operands, the widest being qkv's, the MLP's or a projector's)."""
        widest = max(3 * self.D, self.Hm, self.m.projector_dim if self.m.z_dims else 0)
        return max_tokens(widest, ops.half_dtype(precision or self.m.precision).itemsize, self.T, self.L.ada_rows)

    def saved_activation_bytes(self, B, recompute=None, plan=None, inference=False):
        """Bytes the tape of a training forward at batch B holds from the forward to the backward: the closed form of
        recompute.saved_activation_bytes for this model.  recompute: a SiT.recompute value (None: the model's); plan: the
        FreezePlan (None: that of the parameters' current requires_grad flags, no input gradient); inference: the forward's flag
        (True: no projector runs)."""
        m = self.m
        pl = plan if plan is not None else self.plan_for()
        rc = recomputed_blocks(m.recompute if recompute is None else recompute, pl.save)
        projs = [] if inference else [(B * self.T if m.z_types[j] == "i" else B, m.projector_dim)
                                      for j in range(len(self.tap_depth)) if pl.proj[j]["run"]]
        return saved_activation_bytes(B, self.T, self.D, self.Hm, self.H, self.depth, ops.half_dtype(m.precision).itemsize, pl.save,
                                      rc, self.C, m.input_size, self.L.ada_rows, bool(m.qk_norm), projs)

    def _linear_fwd(self, name, epi, act, M, N, K, C, C2=None, ldc2=0, **kw):
        """The 16-bit forward launch of block linear `name`: the forward's, and the one a recomputed block's rebuild repeats."""
        ops.gemm(NT, epi, act, self.W(name + ".weight"), M, N, K, C, K, K, N, C2=C2, ldc2=ldc2, bias=self.W(name + ".bias"), **kw)

    def forward(self, x, t, y, inference, need_grad, drop, plan=None):
        """plan: the FreezePlan of this forward's backward (need_grad only; None = every block saves, as with every parameter
        trainable)."""
        prec = self.m.precision
        if need_grad and self.m.fp8:
            raise RuntimeError("reed_amd.SiT: fp8 is a sampling mode (inference forward under torch.no_grad()); a forward that "
                               "builds a graph (training, input gradients) needs model.fp8 = False")
        with ops.build(prec, bool(self.m.tf32)):
            return self._forward(x, t, y, inference, need_grad, drop, prec, plan)

    def _forward(self, x, t, y, inference, need_grad, drop, prec, plan=None):
        m, L = self.m, self.L
        ops.require_cuda(x, "x")
        dev = x.device
        B, C, HW = x.shape[0], x.shape[1], x.shape[-1]
        D, H, hd, Hm, T, P = self.D, self.H, self.hd, self.Hm, self.T, self.P
        if C != self.C or HW != m.input_size or x.shape[-2] != HW:
            raise ValueError(f"input {tuple(x.shape)} does not match (N,{self.C},{m.input_size},{m.input_size})")
        M = B * T
        self._check_dims(prec)
        if need_grad and (plan is None or plan.any) and M > self.max_tokens(prec):
            raise ValueError(f"reed_amd.SiT: a training forward of {B} x {T} = {M} tokens is past the {self.max_tokens(prec)} tokens the "
                             f"weight-gradient kernels' 32-bit offsets cover at this width (reed_amd/recompute.py:max_tokens); use a "
                             f"smaller local batch with gradient accumulation")
        self._shadow = self.A.ensure_shadow(prec)
        hdt = ops.half_dtype(prec)
        hb = self._hb = hdt.itemsize    # bytes per element of the operand / activation arrays (2; 4 in the fp32-operand build)
        pend = self.A.pending   # parameter buckets an overlapped optimiser step is still rewriting (optim.py)
        if "all" in pend:
            self.A.wait_all()
        elif pend:
            self.A.wait("embed")
        x = x.contiguous().float()
        t = t.contiguous().float()
        y = y.contiguous().long()
        bf, f32 = _allocators(hdt, dev)
        sag = self.save_act_grad if self.save_act_grad is not None else M > self.SAVE_ACT_GRAD_MIN_TOKENS
        self._sag = sag   # (the projector forward of this call follows it)
        tp = types.SimpleNamespace(B=B, blocks=[], proj={}, x=x, t=t, prec=prec, act_grad=sag, plan=plan) if need_grad else None
        # a partly frozen model (freeze.py): blocks below the lowest one whose backward runs save nothing
        save = plan.save if (need_grad and plan is not None) else [need_grad] * self.depth
        rc = recomputed_blocks(m.recompute, save) if need_grad else [False] * self.depth   # (recompute.py; a bad value raises here)
        # epilogues of a layer whose saved array feeds the backward (gemm.h): derivative-saving forms when there is a backward
        epi_silu = EPI_SILU_G if need_grad and sag else EPI_SILU
        epi_gelu = EPI_GELU_G if need_grad and sag else EPI_GELU
        # -- embedders
        tok = f32(M, D)
        ops.patch_embed_fwd(x, self.W("x_embedder.proj.weight"), self.W("x_embedder.proj.bias"), self.Wf("pos_embed"),
                            tok, B, C, HW, P, D)
        sin = bf(B, 256)
        ops.timestep_sinusoid(t, sin, B)
        t1p = bf(B, D) if need_grad else None
        t1 = bf(B, D)
        ops.gemm(NT, epi_silu, sin, self.W("t_embedder.mlp.0.weight"), B, D, 256, t1p, 256, 256, D, C2=t1, ldc2=D,
                 bias=self.W("t_embedder.mlp.0.bias"))
        temb = bf(B, D)
        ops.gemm(NT, EPI_BF16, t1, self.W("t_embedder.mlp.2.weight"), B, D, D, temb, D, D, D,
                 bias=self.W("t_embedder.mlp.2.bias"))
        drop_u8 = None
        if drop is not None:
            drop_u8 = drop.to(device=dev, dtype=torch.uint8).contiguous()
        labels_eff = torch.empty(B, dtype=torch.int64, device=dev)
        c = f32(B, D)
        silu_c = bf(B, D)
        if self._err is None:
            self._err = torch.zeros(1, dtype=torch.int32, device=dev)
        ops.label_cond(y, drop_u8, m.num_classes, self.Wf("y_embedder.embedding_table.weight"), temb, labels_eff, c,
                       silu_c, B, D, table_rows=self.table_rows, err=self._err)
        Nall = L.ada_rows
        mod = bf(B, Nall)
        sp = self._shadow.data_ptr()
        mp = mod.data_ptr()
        # modulation of every block: one GEMM on silu(c) — or two when an overlapped optimiser step is still rewriting the
        # tail of the adaLN matrix (a third of all parameters): the head blocks' rows now, the rest when block kh starts
        kh = min(L.ADA_HEAD_BLOCKS, self.depth) if "ada_tail" in pend else 0
        n_head = kh * 6 * D if kh else Nall
        if pend:
            self.A.wait("ada_head")
        ops.gemm(NT, EPI_BF16, silu_c, sp + hb * L.ada_w_off, B, n_head, D, mod, D, D, Nall, bias=sp + hb * L.ada_b_off)

        def ada_rest():   # the rest of the modulation rows, once the optimiser has rewritten the tail of the adaLN matrix
            self.A.wait("ada_tail")
            ops.gemm(NT, EPI_BF16, silu_c, sp + hb * (L.ada_w_off + n_head * D), B, Nall - n_head, D, mp + hb * n_head,
                     D, D, Nall, bias=sp + hb * (L.ada_b_off + n_head))
        if need_grad:
            tp.sin, tp.t1p, tp.t1, tp.labels_eff, tp.c, tp.silu_c, tp.mod = sin, t1p, t1, labels_eff, c, silu_c, mod

        # -- blocks
        if not all(save):  # inference, blocks without a backward: ping-pong buffers, nothing saved
            xa, xb = tok, f32(M, D)
            h, qkv, o, u = bf(M, D), bf(M, 3 * D), bf(M, D), bf(M, Hm)
        # fp8 sampling (SiT.fp8; inference branch, 16-bit builds): the block linears that reed_gemm_mxfp8 takes at this token count run
        # on MX-fp8 operands — the activation quantised by a row pass in front of the GEMM, the weight from the arena's quantised
        # copy — each layer decided on its own; everything else, and every other layer, stays on the 16-bit kernels.
        mx_on = ()
        if not need_grad and prec in ("bf16", "fp16") and m.fp8:
            layers = self.fp8_layers(M, prec)
            mx_on = frozenset(n for n, on in layers.items() if on)
            if not self._fp8_logged:
                self._fp8_logged = True
                logger.info("fp8 sampling: MX-fp8 block GEMMs for %s; 16-bit for %s", sorted(mx_on) or "no layer",
                            sorted(n for n, on in layers.items() if not on) or "no layer")
        if mx_on:
            mxw = self.A.ensure_mx(prec)
            kmax = max(D, Hm)
            aq = torch.empty((M, kmax), dtype=torch.uint8, device=dev)
            asc = torch.empty((M, kmax // ops.MX_BLOCK), dtype=torch.uint8, device=dev)

        def linear(lin, epi, act, N, K, C, C2=None, ldc2=0, **kw):
            """The forward of linear `lin` of the block at hand (b), act [M, K] -> C / C2 [M, N] (+ bias; kw: the epilogue's gate and
            residual): the MX-fp8 GEMM where fp8 sampling takes this layer (nothing is saved there, and a null output goes with a
            zero leading dimension), the 16-bit one otherwise."""
            name = b + lin
            if lin in mx_on:
                wq, wsc = mxw[name + ".weight"]
                ops.mx_quantize(act, aq, asc, M, K)
                ops.gemm_mxfp8(epi, aq, asc, wq, wsc, M, N, K, C, N if C is not None else 0, C2=C2,
                               ldc2=ldc2 if C2 is not None else 0, bias=self.W(name + ".bias"), **kw)
            else:
                self._linear_fwd(name, epi, act, M, N, K, C, C2, ldc2, **kw)

        # recompute (recompute.py): the lowest blocks with a backward keep their input and y2 and run like the blocks that save
        # nothing, on shared h / qkv / o / u and one shared xmid; Engine._recompute_block rebuilds their record in the backward
        rc_left = sum(rc)
        if rc_left:
            if all(save):
                h, qkv, o, u = bf(M, D), bf(M, 3 * D), bf(M, D), bf(M, Hm)
            rc_buf = (h, qkv, o, u, f32(M, D))
        xcur = tok
        zs_by_proj = {}
        for i in range(self.depth):
            b = f"blocks.{i}."
            mb = mp + hb * (i * 6 * D)
            if kh and i == kh:
                ada_rest()
                kh = 0
            if pend:
                self.A.wait(f"block{i}")
            keep = save[i] and not rc[i]     # this block's forward saves its activations
            if rc[i]:
                h, qkv, o, u, xmid = rc_buf
                h2, a1, y1, y2 = h, None, None, bf(M, D)
                mean1 = rstd1 = mean2 = rstd2 = lse = None
                xout = f32(M, D)
            elif save[i]:
                h, qkv, o, u = bf(M, D), bf(M, 3 * D), bf(M, D), bf(M, Hm)
                h2, a1, y1, y2 = bf(M, D), bf(M, Hm), bf(M, D), bf(M, D)
                mean1, rstd1, mean2, rstd2 = f32(M), f32(M), f32(M), f32(M)
                lse = f32(B, H, T)
                xmid, xout = f32(M, D), f32(M, D)
            else:
                h2, a1, y1, y2 = h, None, None, None
                mean1 = rstd1 = mean2 = rstd2 = lse = None
                xmid = xb if xcur is xa else xa
                xout = xcur  # safe: fc2's epilogue reads R=xmid, writes xout; xcur is dead after proj
            ops.ln_modulate_fwd(xcur, mb, mb + hb * D, Nall, h, mean1, rstd1, M, D, T)
            linear("attn.qkv", EPI_BF16, h, 3 * D, D, qkv)
            qkv_a, qstats = qkv, None
            if m.qk_norm:
                qkv_a = bf(M, 3 * D)
                qstats = f32(M, 2, H, 2) if keep else None
                ops.qk_norm_fwd(qkv, self.Wf(b + "attn.q_norm.weight"), self.Wf(b + "attn.q_norm.bias"),
                                self.Wf(b + "attn.k_norm.weight"), self.Wf(b + "attn.k_norm.bias"), qkv_a, qstats, M, H, hd)
            ops.attention_fwd(qkv_a, o, lse, B, T, H, hd)
            linear("attn.proj", EPI_GATE_RES, o, D, D, xmid, C2=y1, ldc2=D, R=xcur, ldr=D, gate=mb + 2 * hb * D, ldgate=Nall,
                   rows_per_gate=T)
            ops.ln_modulate_fwd(xmid, mb + 3 * hb * D, mb + 4 * hb * D, Nall, h2, mean2, rstd2, M, D, T)
            linear("mlp.fc1", epi_gelu if keep else EPI_GELU, h2, Hm, D, a1, C2=u, ldc2=Hm)
            linear("mlp.fc2", EPI_GATE_RES, u, D, Hm, xout, C2=y2, ldc2=D, R=xmid, ldr=D, gate=mb + 5 * hb * D, ldgate=Nall,
                   rows_per_gate=T)
            if need_grad and not save[i]:
                tp.blocks.append(None)
            elif rc[i]:
                tp.blocks.append(types.SimpleNamespace(rc=True, x=xcur, y2=y2))
                rc_left -= 1
                if not rc_left:   # the shared buffers go back before the blocks that save allocate theirs
                    rc_buf = h = qkv = o = u = h2 = xmid = qkv_a = None
            elif need_grad:
                tp.blocks.append(types.SimpleNamespace(x=xcur, mean1=mean1, rstd1=rstd1, h=h, qkv=qkv, qkv_a=qkv_a,
                                                       qstats=qstats, o=o, lse=lse,
                                                       y1=y1, xmid=xmid, mean2=mean2, rstd2=rstd2, h2=h2, a1=a1, u=u,
                                                       y2=y2, rc=False))
            xcur = xout
            if not inference:
                for j, dj in enumerate(self.tap_depth):
                    if dj == i + 1:
                        zs_by_proj[j] = self._projector_fwd(j, xcur, B, need_grad and (plan is None or plan.proj[j]["run"]), tp)
        # -- final layer
        if kh:   # depth <= ADA_HEAD_BLOCKS: the tail (final layer's rows) was never launched
            ada_rest()
        if pend:
            self.A.wait_all()
        out = f32(B, C, HW, HW)
        meanF = f32(M) if need_grad else None
        rstdF = f32(M) if need_grad else None
        mf = mp + hb * (self.depth * 6 * D)
        ops.final_layer_fwd(xcur, mf, mf + hb * D, Nall, self.W("final_layer.linear.weight"),
                            self.W("final_layer.linear.bias"), out, meanF, rstdF, B, T, D, C, P)
        if need_grad:
            tp.x_last, tp.meanF, tp.rstdF = xcur, meanF, rstdF
        zs = None
        if not inference:
            if self.split:
                ji, jt = m.z_types.index("i"), m.z_types.index("t")
                zs = [zs_by_proj[ji], zs_by_proj[jt]]
                if need_grad:
                    tp.zs_order = [ji, jt]
            else:
                zs = [zs_by_proj[j] for j in range(len(m.z_dims))]
                if need_grad:
                    tp.zs_order = list(range(len(m.z_dims)))
        return out, zs, tp

    def _projector_fwd(self, j, x, B, need_grad, tp):
        m, D, T = self.m, self.D, self.T
        Pd, Z = m.projector_dim, m.z_dims[j]
        dev = x.device
        img = m.z_types[j] == "i"
        self.A.wait("projectors")
        R = B * T if img else B
        bf, _ = _allocators(ops.half_dtype(), dev)   # the build Engine.forward selected
        xin = bf(R, D)
        if img:
            ops.ln_modulate_fwd(x, None, None, 0, xin, None, None, R, D, T)  # f32 -> bf16 cast (autocast input cast)
        else:
            ops.token_mean_fwd(x, xin, B, T, D)
        pre = f"projectors.{j}."
        epi_silu = EPI_SILU_G if need_grad and self._sag else EPI_SILU
        p1p, p1 = (bf(R, Pd) if need_grad else None), bf(R, Pd)
        ops.gemm(NT, epi_silu, xin, self.W(pre + "0.weight"), R, Pd, D, p1p, D, D, Pd, C2=p1, ldc2=Pd,
                 bias=self.W(pre + "0.bias"))
        p2p, p2 = (bf(R, Pd) if need_grad else None), bf(R, Pd)
        ops.gemm(NT, epi_silu, p1, self.W(pre + "2.weight"), R, Pd, Pd, p2p, Pd, Pd, Pd, C2=p2, ldc2=Pd,
                 bias=self.W(pre + "2.bias"))
        zt = bf(R, Z)
        ops.gemm(NT, EPI_BF16, p2, self.W(pre + "4.weight"), R, Z, Pd, zt, Pd, Pd, Z, bias=self.W(pre + "4.bias"))
        if need_grad:
            tp.proj[j] = types.SimpleNamespace(xin=xin, p1p=p1p, p1=p1, p2p=p2p, p2=p2, R=R)
        return zt.view(B, T, Z) if img else zt

    # ---- backward ------------------------------------------------------------------
    def _wgrad_block(self, probs, Mtok, acc, dev, side):
        """The four weight gradients of a block as one launch without split-K (ops.wgrad_group; csrc/gemm_tn.hip): probs =
        [(dy, x, weight name, n_out, k_in), ...].  Falls back to the per-GEMM path when the device is too small."""
        args = [(dy, x, self.G(w), self.G(w.replace("weight", "bias")), N, K) for dy, x, w, N, K in probs]
        if side is not None:
            side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            done = ops.wgrad_group(args, Mtok, accumulate=acc)
        if not done:
            for dy, x, w, N, K in probs:
                self._wgrad(dy, x, w, Mtok, N, K, acc, dev, side=side)
            return
        if side is not None:
            for dy, x, _, _, _ in probs:
                dy.record_stream(side)
                x.record_stream(side)

    def _wgrad(self, dy, x, wname, Mtok, N, K, acc, dev, bias_done=False, side=None):
        """dW (+)= dy^T x and db (+)= colsum(dy) into the gradient arena: the TN kernel / tile ops.plan_wgrad picks
        (256x128, 128x256 or 128x128) with wave-quantised split-K through slabs (deterministic reduce); the bias gradient rides along as an extra
        ones-MFMA in the blocks of the first column tile unless the caller already has it (bias_done).
        side = the weight-gradient stream: the launch is ordered after everything queued on the current stream so far
        (dy is the newest tensor it reads) and runs beside the dgrad chain, which nothing downstream of it in
        backward depends on — it fills the CUs the chain's ragged last tile rounds leave idle (at b = 32/GPU a
        256-row-tile dgrad grid covers 56-84 % of the 256 CUs)."""
        bname = wname.replace("weight", "bias")
        lay, split = ops.plan_wgrad(Mtok, N, K)
        if side is not None:
            side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            # (the side stream's split-K slabs are its own: allocated while that stream is current)
            ws = (self.ws if side is None else self.ws_side)(split * (N * K + N), dev) if split > 1 else None
            ops.linear_wgrad(dy, x, self.G(wname), dbias=None if bias_done else self.G(bname), accumulate=acc,
                             split_k=split, Mtok=Mtok, N=N, K=K, ws=ws, lay=lay)
        if side is not None:
            dy.record_stream(side)   # allocated on the main stream: the caching allocator must not hand these
            x.record_stream(side)    # blocks out again before the side stream's reads have finished

    def _lora_grads(self, dy, x, lin, Mtok, N, K, acc, dev):
        """The gradients of the adapters of linear `lin` from its (dy, x) pair (csrc/lora.hip), on the current stream: the 16-bit
        adapters come from the shadow, the gradients go to the arena like every other parameter's."""
        R = self.m.lora_rank
        ws = self.ws(ops.lora_grads_ws_floats(Mtok, N, K, R), dev)
        ops.lora_grads(x, dy, self.W(lin + ".lora_A"), self.W(lin + ".lora_B"), self.L.lora_scale, self.G(lin + ".lora_A"),
                       self.G(lin + ".lora_B"), ws, Mtok, N, K, R, acc)

    def WT(self, name):
        """Device address of the transposed 16-bit copy W^T [k_in, n_out] of a block linear's weight (arena.py), or None."""
        if self._shadow_t is None:
            return None
        seg = self.A.t_seg.get(name)
        return None if seg is None else self._shadow_t.data_ptr() + self._hb * seg[0]

    def _dgrad(self, epi, dy, wname, Mtok, N, K, out, **kw):
        """dx[Mtok,K] = dy[Mtok,N] W[N,K].  With the transposed copy of the weight (round 6: the blocks' linears above
        DGRAD_NT_MIN_TOKENS) an NT GEMM on W^T — both operands k-contiguous; otherwise NN straight on the weight shadow (W is the
        k-strided operand, read with transposing LDS reads).  The same products in the same order: the same bits."""
        wt = self.WT(wname)
        if wt is not None:
            ops.gemm(NT, epi, dy, wt, Mtok, K, N, out, N, N, K, **kw)
        else:
            ops.gemm(NN, epi, dy, self.W(wname), Mtok, K, N, out, N, K, K, **kw)

    def backward(self, tp, dout, dzs, need_x=False, need_t=False, frozen=False):
        """Parameter gradients into the gradient arena; returns (dL/dx f32 [B, C, HW, HW] | None, dL/dt f32 [B] | None), each
        computed only when asked for (need_x / need_t).  frozen: no parameter requires grad — the activation-gradient chain alone
        (the same launches in the same order: dx and dt have the bits of the full backward), no weight or bias gradient, no
        gradient arena."""
        prec = self.m.precision
        if tp.prec != prec:
            raise RuntimeError("reed_amd.SiT: model.precision changed between forward and backward")
        if tp.plan is not None and tp.plan.sig != self.signature():
            raise RuntimeError("reed_amd.SiT: a parameter's requires_grad changed between forward and backward; the forward saved "
                               "what the plan of that moment needs (reed_amd/freeze.py). Run the forward again")
        if frozen and self.reducer is not None:
            raise RuntimeError(FROZEN_WITH_REDUCER)
        with ops.build(prec, bool(self.m.tf32)):
            # gradient buckets are reduced beside this backward's GEMMs (RCCL channels hold CUs): only then does the library keep to
            # kernels that degrade gracefully without every CU (csrc/gemm_plan.cpp:reed_set_concurrent_comm); the forward, the
            # optimiser and the sampler run with no collective in flight (the step waits for the last bucket before the update)
            comm = self.reducer is not None and self.reducer.active()
            if comm:
                ops.set_concurrent_comm(True)
            try:
                return self._backward(tp, dout, dzs, need_x, need_t, not frozen)
            finally:
                if comm:
                    ops.set_concurrent_comm(False)

    def _backward(self, tp, dout, dzs, need_x, need_t, wgrads):
        """wgrads = False (the frozen-weight backward): every launch that only feeds a parameter gradient is skipped; what is
        left runs as it does with them.  In between, the tape's FreezePlan (freeze.py) decides launch by launch, and where the
        activation-gradient chain stops.  The phases, in order: _backward_final, per block from the top down to pl.k the projector
        taps of its output and _backward_block, _backward_truncated_end (a truncated backward's low projectors), _backward_tail,
        _backward_end; `s` is the per-call record they share."""
        pl = tp.plan if tp.plan is not None else self.plan_for(need_x, need_t)
        D, H, Hm, T = self.D, self.H, self.Hm, self.T
        B = tp.B
        M = B * T
        dev = dout.device
        hdt = ops.half_dtype(tp.prec)
        hb = self._hb = hdt.itemsize
        if wgrads:
            self.A.ensure_grad()
        # the transposed copies of the blocks' weights (the dgrads' NT operand): built on first use, then kept fresh by the optimiser
        use_t = self.dgrad_nt if self.dgrad_nt is not None else (self.DGRAD_NT_MIN_TOKENS is not None and M >= self.DGRAD_NT_MIN_TOKENS)
        self._shadow_t = self.A.ensure_shadow_t(tp.prec) if (use_t and hb == 2) else None
        acc = self.grad_live
        bf, f32 = _allocators(hdt, dev)
        red = self.reducer
        reducing = red is not None and red.active()
        group = wgrads and any(pl.group) and ops.wgrad_group_fits([(D, Hm), (Hm, D), (D, D), (3 * D, D)])
        nws = ops.attention_bwd_ws_floats(B, T, H)       # delta = rowsum(dO * O) of the persistent attention backward
        attn_ws = f32(nws) if nws else None
        # the answer of the library ("this shape's dO GEMM has the head-dot epilogue") depends on which kernel the GEMM runs on:
        # the token count, the operand type, whether gradient buckets are being reduced beside this backward (the library then
        # keeps off the persistent kernels) and a forced tile — all in the key (a 1002 seen once under one of
        # them was remembered for the rest of the run under the token count alone).
        # (and the CU reserve and the forms-beside-collectives switch, which the tuner cycles under one token count)
        # (and whether that GEMM is the NT one on the transposed weights or the NN one: two shapes to the planner)
        dkey = (M, str(hdt), reducing, ops.gemm_forced_tile(), ops.cu_reserve(), ops.comm_forms(), self._shadow_t is not None)
        side = None
        if wgrads and (self.wgrad_stream or (self.wgrad_stream is None and M <= self.wgrad_stream_max_tokens)):
            if self._side is None:
                self._side = torch.cuda.Stream(device=dev)
            side = self._side
        # With a reducer attached the adaLN weight gradient is computed block by block (rows of block i right after
        # block i's backward: dW_ada[i] = dmod[:, i]^T silu(c), a K = b GEMM) instead of one GEMM at the end, so each
        # slice's all-reduce overlaps the rest of backward; the arithmetic per output element is the same.
        split_ada = pl.any_ada and (red is not None if self.split_ada_wgrad is None else self.split_ada_wgrad)
        # Factor path (a reducer that is reducing THIS backward, no gradient accumulation in flight): the adaLN weight
        # gradient contracts over the local batch only, so instead of all-reducing the [Nall, D] fp32 matrix (a third of
        # the payload) the ranks all-gather the two bf16 factors — dmod rows of block i (pre-scaled by 1 / world: exact,
        # power-of-two worlds only) right after block i's backward, silu(c) once — and every rank forms the global-batch
        # product itself at the end of backward (K = world * b). At world = 1 this is the per-block GEMM on a copy.
        fg = (reducing and red.ada_gather and not acc and self.split_ada_wgrad is None and wgrads
              and not pl.trunc)   # (truncated: the all-reduced per-block slices; the same plan on every rank)
        dz = {j: dzs[k] for k, j in enumerate(tp.zs_order)} if dzs is not None else {}
        s = types.SimpleNamespace(tp=tp, pl=pl, wgrads=wgrads, acc=acc, side=side, dev=dev, bf=bf, f32=f32, B=B, M=M, hb=hb,
                                  Nall=self.L.ada_rows, mp=tp.mod.data_ptr(), group=group, attn_ws=attn_ws, dkey=dkey,
                                  dot_delta=self._dot_delta if self.fused_delta and hdt != torch.float32 else {dkey: False},
                                  fg=fg, split_ada=split_ada and not fg, gp=self.A.grad.data_ptr() if wgrads else None, dz=dz,
                                  dx=None, dmod=None, pre=None, g_send=None, g_recv=None, s_all=None)
        self.recomputed = 0
        self._backward_final(s, dout.contiguous().float())
        proj_left = len(tp.proj)
        proj_fired = False
        for i in reversed(range(pl.k, self.depth)):
            for j, dj in enumerate(self.tap_depth):   # which projectors fire after block i's output?
                if dj == i + 1 and j in tp.proj:
                    self._projector_bwd(j, tp, dz.get(j), s.dx, B, acc, dev, pl.proj[j])
                    proj_left -= 1
                    if proj_left == 0 and red is not None:
                        red.ready("projectors")
                        proj_fired = True
            self._backward_block(s, i)
        if pl.trunc:
            self._backward_truncated_end(s)
        return self._backward_end(s, self._backward_tail(s), proj_fired, need_x, need_t)

    def _ln_bwd(self, s, dh, x, mean, rstd, scale_ptr, part, nxt):
        """LayerNorm+modulate backward into dx. nxt = index of the block whose MLP-branch gate consumes the finished
        dx next: its gate backward rides along in the same pass unless that block does not run or a projector tap adds
        into dx in between (a projector backward adds into dx between block nxt and nxt + 1). Returns (dy2, pg2) of that block
        when fused."""
        tp, M, D, T, Nall = s.tp, s.M, self.D, self.T, s.Nall
        if nxt < s.pl.k or any(dj == nxt + 1 and j in tp.proj for j, dj in enumerate(self.tap_depth)):
            ops.ln_modulate_bwd(dh, x, mean, rstd, scale_ptr, Nall, s.dx, part, M, D, T)
            return None
        dy, pg = s.bf(M, D), s.f32(M // 16, D)
        ops.ln_modulate_bwd_gate(dh, x, mean, rstd, scale_ptr, Nall, s.dx, part, tp.blocks[nxt].y2,
                                 s.mp + s.hb * (nxt * 6 * D + 5 * D), Nall, dy, pg, None, M, D, T)
        return dy, pg

    def _ada_rows(self, i):
        """(first row, rows) of block i's part of the stacked adaLN matrix; i = depth: the final layer's."""
        return i * 6 * self.D, (6 * self.D if i < self.depth else 2 * self.D)

    def _ada_after(self, s, i):
        """Block i's dmod rows are final: on the factor path scale them, pack them [b, rows] contiguously and all-gather; with the
        adaLN weight gradient block by block, its rows' GEMM where they are trainable."""
        if not (s.fg or (s.split_ada and s.pl.ada[i])):
            return
        L, D, B = self.L, self.D, s.B
        c0, rows = self._ada_rows(i)
        if s.fg:
            W = self.reducer.world
            snd = s.g_send[B * c0:B * (c0 + rows)]
            torch.mul(s.dmod[:, c0:c0 + rows], 1.0 / W, out=snd.view(B, rows))
            self.reducer.gather(snd, s.g_recv[W * B * c0:W * B * (c0 + rows)])
        else:
            ops.gemm(TN, EPI_F32, s.dmod.data_ptr() + s.hb * c0, s.tp.silu_c, rows, D, B, s.gp + 4 * (L.ada_w_off + c0 * D),
                     s.Nall, D, D, dbias=s.gp + 4 * (L.ada_b_off + c0), accumulate=s.acc)

    def _fire(self, s, name, i, side=None):
        """Hand gradient bucket `name` to the reducer and, where the adaLN weight gradient goes block by block, ada{i} with it.
        side: the bucket holds gradients written on both streams: fire it from the side stream, after main."""
        red = self.reducer
        if red is None:
            return
        if side is not None:
            side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
            red.ready(name)
            if s.split_ada:
                red.ready(f"ada{i}")

    def _backward_final(self, s, dout):
        """The final layer: its row kernel, its LayerNorm backward — which starts dx, the gradient of the residual stream — and its
        linear's gradients; the modulation gradients' array with the final layer's rows, and the first buckets."""
        tp, pl, bf, f32 = s.tp, s.pl, s.bf, s.f32
        D, T, P, C, depth = self.D, self.T, self.P, self.C, self.depth
        B, M, hb, Nall, dev = s.B, s.M, s.hb, s.Nall, s.dev
        mf = s.mp + hb * (depth * 6 * D)
        if pl.final_run:
            hbuf, dlin, dh = bf(M, D), bf(M, self.NO), bf(M, D)
            ops.final_layer_bwd_rows(dout, tp.x_last, tp.meanF, tp.rstdF, mf, mf + hb * D, Nall,
                                     self.W("final_layer.linear.weight"), hbuf, dlin, dh, B, T, D, C, P)
        if pl.final_ln:
            s.dx = torch.zeros(M, D, dtype=torch.float32, device=dev)
            partF = f32(M // 16, 2, D)
            s.pre = self._ln_bwd(s, dh, tp.x_last, tp.meanF, tp.rstdF, mf + hb * D, partF, depth - 1)
        if pl.final_w:
            wsf = self.ws(ops.smallk_ws_floats(D, max(self.NO, C * P * P)), dev)
            ops.smallk_wgrad(hbuf, False, dlin, wsf, self.G("final_layer.linear.weight"), None,
                             self.G("final_layer.linear.bias"), M, D, self.NO, 1, s.acc)
        # the modulation gradients of every block + the final layer; truncated, only trainable adaLN rows are reduced into it and
        # the stacked weight-gradient GEMM reads zeros elsewhere
        if pl.dmod:
            s.dmod = torch.zeros(B, Nall, dtype=tp.mod.dtype, device=dev) if pl.trunc else bf(B, Nall)
        offF = depth * 6 * D
        if pl.final_ln and pl.mod_reduce[depth]:
            ops.reduce_mod_parts([(partF.data_ptr(), 2 * D, offF), (partF.data_ptr() + 4 * D, 2 * D, offF + D)], s.dmod, Nall,
                                 B, D, T // 16)
        if pl.final_run:
            del hbuf, dlin, dh
        if s.fg:
            red = self.reducer
            s.g_send, s.g_recv = red.gather_buffers("dmod", B * Nall, tp.mod.dtype, dev)
            s_send, s.s_all = red.gather_buffers("silu", B * D, tp.mod.dtype, dev)
            s_send.view(B, D).copy_(tp.silu_c)
            red.gather(s_send, s.s_all)
        self._ada_after(s, depth)
        self._fire(s, "final", depth)

    def _lin_grads(self, s, i, wg, lin, dy, x, N, K):
        """The parameter gradients of linear `lin` of block i from its (dy, x) pair, as the plan says (freeze.py: group / lin /
        lora): the weight and bias gradient joins the block's one launch (wg: it goes out with the last linear) or takes a launch
        of its own; the adapters' gradients follow.
        (bias gradients of fc2 / proj = column sums of dy2 / dy1: fused into their weight-gradient GEMMs)"""
        name = f"blocks.{i}.{lin}"
        if wg is not None:
            wg.append((dy, x, name + ".weight", N, K))
            if lin == LINEARS[-1]:
                self._wgrad_block(wg, s.M, s.acc, s.dev, s.side)
        elif s.pl.lin[i][lin]:
            self._wgrad(dy, x, name + ".weight", s.M, N, K, s.acc, s.dev, side=s.side)
        if s.wgrads and s.pl.lora[i][lin]:
            self._lora_grads(dy, x, name, s.M, N, K, s.acc, s.dev)

    def _recompute_block(self, s, i, ck):
        """The record a saving forward leaves of block i, rebuilt from its checkpoint ck (x, y2): the forward's launches up to fc1
        with the forward's arguments — the same kernels on the same operands, the same bits; fc2 is not run, its one saved output
        is ck.y2.  fc1's epilogue is the one the tape's forward would have used (tp.act_grad)."""
        tp, bf, f32 = s.tp, s.bf, s.f32
        D, H, hd, Hm, T = self.D, self.H, self.hd, self.Hm, self.T
        B, M, hb, Nall = s.B, s.M, s.hb, s.Nall
        b = f"blocks.{i}."
        mb = s.mp + hb * (i * 6 * D)
        h, qkv, o, u = bf(M, D), bf(M, 3 * D), bf(M, D), bf(M, Hm)
        h2, a1, y1 = bf(M, D), bf(M, Hm), bf(M, D)
        mean1, rstd1, mean2, rstd2 = f32(M), f32(M), f32(M), f32(M)
        lse = f32(B, H, T)
        xmid = f32(M, D)
        ops.ln_modulate_fwd(ck.x, mb, mb + hb * D, Nall, h, mean1, rstd1, M, D, T)
        self._linear_fwd(b + "attn.qkv", EPI_BF16, h, M, 3 * D, D, qkv)
        qkv_a, qstats = qkv, None
        if self.m.qk_norm:
            qkv_a = bf(M, 3 * D)
            qstats = f32(M, 2, H, 2)
            ops.qk_norm_fwd(qkv, self.Wf(b + "attn.q_norm.weight"), self.Wf(b + "attn.q_norm.bias"),
                            self.Wf(b + "attn.k_norm.weight"), self.Wf(b + "attn.k_norm.bias"), qkv_a, qstats, M, H, hd)
        ops.attention_fwd(qkv_a, o, lse, B, T, H, hd)
        self._linear_fwd(b + "attn.proj", EPI_GATE_RES, o, M, D, D, xmid, C2=y1, ldc2=D, R=ck.x, ldr=D, gate=mb + 2 * hb * D,
                         ldgate=Nall, rows_per_gate=T)
        ops.ln_modulate_fwd(xmid, mb + 3 * hb * D, mb + 4 * hb * D, Nall, h2, mean2, rstd2, M, D, T)
        self._linear_fwd(b + "mlp.fc1", EPI_GELU_G if tp.act_grad else EPI_GELU, h2, M, Hm, D, a1, C2=u, ldc2=Hm)
        self.recomputed += 1
        return types.SimpleNamespace(x=ck.x, mean1=mean1, rstd1=rstd1, h=h, qkv=qkv, qkv_a=qkv_a, qstats=qstats, o=o, lse=lse,
                                     y1=y1, xmid=xmid, mean2=mean2, rstd2=rstd2, h2=h2, a1=a1, u=u, y2=ck.y2, rc=False)

    def _backward_block(self, s, i):
        """Block i's backward: stages 1 .. pl.stage[i] of freeze.py, then its adaLN rows and its gradient bucket."""
        tp, pl, bf, f32 = s.tp, s.pl, s.bf, s.f32
        D, H, hd, Hm, T = self.D, self.H, self.hd, self.Hm, self.T
        B, M, hb, Nall, dx, side = s.B, s.M, s.hb, s.Nall, s.dx, s.side
        bk = tp.blocks[i]
        if bk.rc:   # a checkpoint (recompute.py): the full record, rebuilt now and released with the block like a saved one
            bk = tp.blocks[i] = self._recompute_block(s, i, bk)
        b = f"blocks.{i}."
        mb = s.mp + hb * (i * 6 * D)
        last = pl.stage[i]   # the stage this block's backward stops behind
        # MLP branch (its gate backward usually came with the previous LayerNorm backward)
        if s.pre is not None:
            dy2, pg2 = s.pre
        else:
            pg2, dy2 = f32(M // 16, D), bf(M, D)
            ops.gate_bwd(dx, bk.y2, mb + 5 * hb * D, Nall, dy2, pg2, M, D, T)
        s.pre = None
        # the block's four weight gradients: one launch at the end of the block where all four are wanted
        wg = [] if s.group and pl.group[i] else None
        self._lin_grads(s, i, wg, "mlp.fc2", dy2, bk.u, D, Hm)
        if last >= 2:
            da1 = bf(M, Hm)
            self._dgrad(EPI_MUL if tp.act_grad else EPI_DGELU, dy2, b + "mlp.fc2.weight", M, D, Hm, da1, R=bk.a1, ldr=Hm)
            self._lin_grads(s, i, wg, "mlp.fc1", da1, bk.h2, Hm, D)
        if last >= 3:
            # reuse dy2 unless its weight gradient (side stream / grouped launch) may still have to read it
            dh2 = dy2 if side is None and wg is None else bf(M, D)
            self._dgrad(EPI_BF16, da1, b + "mlp.fc1.weight", M, Hm, D, dh2)
            # LN2 backward + the attention branch's gate backward in one pass over dx
            pl2 = f32(M // 16, 2, D)
            pg1, dy1 = f32(M // 16, D), bf(M, D)
            ops.ln_modulate_bwd_gate(dh2, bk.xmid, bk.mean2, bk.rstd2, mb + 4 * hb * D, Nall, dx, pl2, bk.y1, mb + 2 * hb * D, Nall,
                                     dy1, pg1, None, M, D, T)
            self._lin_grads(s, i, wg, "attn.proj", dy1, bk.o, D, D)
        if last >= 4:
            do = bf(M, D)
            dqkv = bf(M, 3 * D)
            # delta = rowsum(dO * O) of the attention backward where dO is produced: the GEMM's epilogue 13 leaves per-row,
            # per-head partial dot products with O (12 MB instead of a 302 MB row pass over dO and O at b = 256); where this
            # shape's GEMM kernel has no such epilogue (False, decided once per token count) the plain store + the row kernel
            fused = False
            if s.dot_delta.get(s.dkey, True) and s.attn_ws is not None:
                dpart = f32(M * H * (1 if hd == 64 else 2))
                fused = s.dot_delta[s.dkey] = ops.dgrad_with_head_dots(dy1, self.W(b + "attn.proj.weight"), do, bk.o, dpart, M, D, D,
                                                                       hd, wt=self.WT(b + "attn.proj.weight"))
            if fused:
                ops.attention_bwd_dp(bk.qkv_a, do, bk.lse, dpart, dqkv, s.attn_ws, B, T, H, hd)
            else:
                self._dgrad(EPI_BF16, dy1, b + "attn.proj.weight", M, D, D, do)
                ops.attention_bwd(bk.qkv_a, bk.o, do, bk.lse, dqkv, B, T, H, hd, ws=s.attn_ws)
            if self.m.qk_norm:  # back through the per-head LayerNorm of q and k; parameter grads via per-block partials
                nb = (M * 3 * H + 255) // 256
                part = f32(nb, 4 * hd)
                dpre = bf(M, 3 * D)
                ops.qk_norm_bwd(dqkv, bk.qkv, bk.qstats, self.Wf(b + "attn.q_norm.weight"),
                                self.Wf(b + "attn.k_norm.weight"), dpre, part, M, H, hd)
                if pl.qknorm[i]:
                    ops.rowsum_f32(part, nb, self.G(b + "attn.q_norm.weight"), 4 * hd, s.acc,
                                   ws=self.ws((nb + 63) // 64 * 4 * hd, s.dev))
                dqkv = dpre
            self._lin_grads(s, i, wg, "attn.qkv", dqkv, bk.h, 3 * D, D)
        if last >= 5:
            dh1 = do  # reuse
            self._dgrad(EPI_BF16, dqkv, b + "attn.qkv.weight", M, 3 * D, D, dh1)
            pl1 = f32(M // 16, 2, D)
            s.pre = self._ln_bwd(s, dh1, bk.x, bk.mean1, bk.rstd1, mb + hb * D, pl1, i - 1)
            if pl.mod_reduce[i]:
                o6 = i * 6 * D
                p1, p2 = pl1.data_ptr(), pl2.data_ptr()
                ops.reduce_mod_parts([(p1, 2 * D, o6), (p1 + 4 * D, 2 * D, o6 + D), (pg1.data_ptr(), D, o6 + 2 * D),
                                      (p2, 2 * D, o6 + 3 * D), (p2 + 4 * D, 2 * D, o6 + 4 * D),
                                      (pg2.data_ptr(), D, o6 + 5 * D)], s.dmod, Nall, B, D, T // 16)
        tp.blocks[i] = None  # free this block's activations
        self._ada_after(s, i)
        self._fire(s, f"block{i}", i, side)

    def _backward_truncated_end(self, s):
        """What only a truncated backward (FreezePlan.trunc) has: the projector chains whose tap lies at or below the lowest block
        that ran (weight gradients only: nothing consumes their dx)."""
        for j, dj in sorted(enumerate(self.tap_depth), key=lambda it: -it[1]):
            if dj <= s.pl.k and s.tp.proj.get(j) is not None:
                self._projector_bwd(j, s.tp, s.dz.get(j), None, s.B, s.acc, s.dev, s.pl.proj[j])

    def _backward_tail(self, s):
        """adaLN (all blocks + final): dW = dmod^T silu(c) — unless it went block by block — and, where the chain runs on
        (not truncated), d silu(c) = dmod @ W (one GEMM each), the conditioning (label table + timestep MLP) and the patch
        embedder.  Returns dt1, the gradient at the timestep MLP's first layer (None: truncated)."""
        tp, pl, L, bf, f32 = s.tp, s.pl, self.L, s.bf, s.f32
        D, P, C = self.D, self.P, self.C
        B, M, hb, Nall, acc, dev, gp, dmod = s.B, s.M, s.hb, s.Nall, s.acc, s.dev, s.gp, s.dmod
        if s.fg:
            self.reducer.gather_sync()
            W = self.reducer.world
            for i in reversed(range(self.depth + 1)):   # rank-major [world * b, rows] factors: K = the global batch
                c0, rows = self._ada_rows(i)
                ops.gemm(TN, EPI_F32, s.g_recv.data_ptr() + hb * W * B * c0, s.s_all, rows, D, W * B,
                         gp + 4 * (L.ada_w_off + c0 * D), rows, D, D, dbias=gp + 4 * (L.ada_b_off + c0), accumulate=False)
        elif pl.any_ada and not s.split_ada:
            ops.gemm(TN, EPI_F32, dmod, tp.silu_c, Nall, D, B, gp + 4 * L.ada_w_off, Nall, D, D,
                     dbias=gp + 4 * L.ada_b_off, accumulate=acc)
        if pl.trunc:
            return None
        ksteps = Nall // 64
        split = min(64, max(1, ksteps // 8))
        slab = B * D
        wsd = self.ws(split * slab, dev)
        ops.gemm(NN, EPI_F32, dmod, self._shadow.data_ptr() + hb * L.ada_w_off, B, D, Nall, wsd, Nall, D, D, split_k=split,
                 slab_stride=slab)
        per = (ksteps + split - 1) // split
        eff = (ksteps + per - 1) // per
        dsilu = f32(B, D)
        ops.reduce_slabs(wsd, slab, eff, dsilu, slab, False)
        # -- conditioning: label table + timestep MLP
        dtemb = bf(B, D)
        gt = None   # a frozen table: no scatter
        if pl.label:
            gt = self.A.view(self.A.grad, "y_embedder.embedding_table.weight")
            if not acc:
                gt.zero_()
        ops.label_cond_bwd(dsilu, tp.c, tp.labels_eff, dtemb, gt, B, D)
        if pl.t2:
            ops.linear_wgrad(dtemb, tp.t1, self.G("t_embedder.mlp.2.weight"), dbias=self.G("t_embedder.mlp.2.bias"),
                             accumulate=acc, Mtok=B, N=D, K=D)
        dt1 = bf(B, D)
        ops.gemm(NN, EPI_MUL if tp.act_grad else EPI_DSILU, dtemb, self.W("t_embedder.mlp.2.weight"), B, D, D, dt1, D, D, D, R=tp.t1p, ldr=D)
        if pl.t0:
            ops.linear_wgrad(dt1, tp.sin, self.G("t_embedder.mlp.0.weight"), dbias=self.G("t_embedder.mlp.0.bias"),
                             accumulate=acc, Mtok=B, N=D, K=256)
        if pl.x_emb:
            # -- patch embed: dW[d,k] = sum_tokens bf16(dx)[token,d] * patch[token,k]
            K = C * P * P
            xb = bf(M, K)
            ops.patchify_bf16(tp.x, xb, B, C, tp.x.shape[-1], P, 0)
            wsf = self.ws(ops.smallk_ws_floats(D, max(self.NO, K)), dev)
            ops.smallk_wgrad(s.dx, True, xb, wsf, self.G("x_embedder.proj.weight"), self.G("x_embedder.proj.bias"), None, M, D,
                             K, 0, acc)
        return dt1

    def _backward_inputs(self, s, dt1, need_x, need_t):
        """The inputs' gradients, after everything they depend on: dL/dt through the sinusoid from dsin = dt1 @ W0 (fp32 out: not
        rounded again), dL/dx = the convolution's input gradient of the finished token gradient."""
        tp, B, D = s.tp, s.B, self.D
        dt_in = dx_in = None
        if need_t:
            dsin = s.f32(B, 256)
            ops.gemm(NN, EPI_F32, dt1, self.W("t_embedder.mlp.0.weight"), B, 256, D, dsin, D, 256, 256)
            dt_in = s.f32(B)
            ops.timestep_sinusoid_bwd(tp.t, dsin, dt_in, B)
        if need_x:
            dx_in = torch.empty_like(tp.x)
            ops.patch_embed_bwd_x(s.dx, self.W("x_embedder.proj.weight"), dx_in, B, self.C, tp.x.shape[-1], self.P, D)
        return dx_in, dt_in

    def _backward_end(self, s, dt1, proj_fired, need_x, need_t):
        """The one end of every backward: the gradient buckets nothing has fired yet, in the reducer's fixed order (the blocks
        below a truncated backward, the projectors where the loop did not reach the last of them, the adaLN slices unless they
        went block by block, the embedders), the inputs' gradients, the side stream's join; returns (dL/dx, dL/dt)."""
        red = self.reducer
        if red is not None:
            for i in reversed(range(s.pl.k)):
                self._fire(s, f"block{i}", i)
            if self.m.z_dims and not proj_fired and hasattr(s.tp, "zs_order"):
                red.ready("projectors")
            if s.fg:   # adaLN weights and biases are global-batch averages already: reduce only the embedders' part
                red.ready_range(self.L.ada_b_off + s.Nall, red.buckets["embed"][1])
            else:
                if not s.split_ada:
                    for i in reversed(range(self.depth + 1)):
                        red.ready(f"ada{i}")
                red.ready("embed")
        grads = self._backward_inputs(s, dt1, need_x, need_t)
        if s.side is not None:  # the optimiser / next micro-step (same stream as this backward) sees every weight gradient
            torch.cuda.current_stream().wait_stream(s.side)
        if s.wgrads:
            self.grad_live = True
            self._attach_grads()
        return grads

    def _projector_bwd(self, j, tp, dz, dx, B, acc, dev, pj=None):
        """pj: the plan's entry for this projector (freeze.py) — which layers want their weight gradient, the layer the chain
        stops behind, whether the tap's contribution to the trunk's dx is formed; None = everything."""
        m, D, T = self.m, self.D, self.T
        Pd, Z = m.projector_dim, m.z_dims[j]
        pr = tp.proj[j]
        R = pr.R
        pre = f"projectors.{j}."
        w = pj["w"] if pj is not None else {4: True, 2: True, 0: True}
        stop = pj["stop"] if pj is not None else -1
        if dz is None:  # projector output unused by the loss: zero grads (torch would leave them None)
            if any(w.values()) and not acc:
                b, e = self.L.range_of(pre)
                self.A.grad[b:e].zero_()
            return
        dz = dz.reshape(R, Z)
        hdt = ops.half_dtype()   # the build Engine.backward selected
        if dz.dtype != hdt:
            dz = dz.to(hdt)
        dz = dz.contiguous()
        bf, _ = _allocators(hdt, dev)
        tp.proj[j] = None
        if w[4]:
            self._wgrad(dz, pr.p2, pre + "4.weight", R, Z, Pd, acc, dev)
        if stop == 4:
            return
        d2 = bf(R, Pd)
        epi_dsilu = EPI_MUL if tp.act_grad else EPI_DSILU
        ops.gemm(NN, epi_dsilu, dz, self.W(pre + "4.weight"), R, Pd, Z, d2, Z, Pd, Pd, R=pr.p2p, ldr=Pd)
        if w[2]:
            self._wgrad(d2, pr.p1, pre + "2.weight", R, Pd, Pd, acc, dev)
        if stop == 2:
            return
        d1 = bf(R, Pd)
        ops.gemm(NN, epi_dsilu, d2, self.W(pre + "2.weight"), R, Pd, Pd, d1, Pd, Pd, Pd, R=pr.p1p, ldr=Pd)
        if w[0]:
            self._wgrad(d1, pr.xin, pre + "0.weight", R, Pd, D, acc, dev)
        if stop == 0:
            return
        if m.z_types[j] == "i":
            ops.gemm(NN, EPI_ADDF32_RB, d1, self.W(pre + "0.weight"), R, D, Pd, dx, Pd, D, D)
        else:
            dmean = bf(R, D)
            ops.gemm(NN, EPI_BF16, d1, self.W(pre + "0.weight"), R, D, Pd, dmean, Pd, D, D)
            ops.token_mean_bwd(dmean, dx, B, T, D)

    def _params(self):
        if self._named is None:   # named_parameters() walks the module tree (1 ms per call on SiT-XL/2): once
            self._named = [(name, p) for name, p in self.m.named_parameters()]
        return self._named

    def signature(self):
        """requires_grad of every named parameter, read afresh from the cached parameter list (no walk over the module tree)."""
        return tuple(p.requires_grad for _, p in self._params())

    def any_trainable(self):
        """Whether any parameter requires grad (pos_embed never does)."""
        return any(self.signature())

    def plan_for(self, need_x=False, need_t=False, sig=None):
        """The FreezePlan (freeze.py) of the parameters' current requires_grad flags, cached per signature."""
        sig = self.signature() if sig is None else sig
        key = (sig, bool(need_x), bool(need_t))
        plan = self._plans.get(key)
        if plan is None:
            names = [n for n, _ in self._params()]
            plan = FreezePlan(self.depth, self.tap_depth, [n for n, on in zip(names, sig) if on], qk_norm=bool(self.m.qk_norm),
                              need_x=need_x, need_t=need_t, all_names=names)
            plan.sig = sig
            plan.first = next((k for k, on in enumerate(sig) if on), None)   # a trainable parameter: its .grad tells whether
            if len(self._plans) > 64:                                          # the caller dropped the gradients
                self._plans.clear()
            self._plans[key] = plan
        return plan

    def _attach_grads(self):
        """Expose the grad arena through param.grad (views), for torch.optim / clip_grad_norm_ compatibility."""
        g = self.A.grad
        for name, p in self._params():
            if p.requires_grad and p.grad is None:
                p.grad = self.A.view(g, name)

    def zero_grad(self):
        """Equivalent of optimizer.zero_grad(set_to_none=True): the next backward overwrites."""
        self.grad_live = False


FROZEN_WITH_REDUCER = ("reed_amd.SiT: an input requires grad while no parameter does (the frozen-weight backward), and a gradient "
                       "reducer is attached to this model: the reducer waits for parameter gradients that backward never writes. "
                       "Detach the reducer, or leave the parameters trainable.")


class _SiTFunction(torch.autograd.Function):
    """anchor: a one-element leaf that requires grad, so that a graph exists when only the parameters (arena views the Function
    never sees as inputs) do; None in the frozen-weight mode, where x or t carries the graph."""

    @staticmethod
    def forward(ctx, anchor, model, x, t, y, inference, drop, plan):
        eng = model.engine()
        out, zs, tape = eng.forward(x, t, y, inference, True, drop, plan)
        ctx.eng, ctx.tape, ctx.frozen = eng, tape, anchor is None
        ctx.nz = 0 if zs is None else len(zs)
        ctx.set_materialize_grads(False)
        return (out,) + (tuple(zs) if zs else ())

    @staticmethod
    def backward(ctx, dout, *dzs):
        if ctx.tape is None:
            raise RuntimeError("reed_amd.SiT: backward called twice on the same forward")
        eng, tape = ctx.eng, ctx.tape
        ctx.tape = None
        if dout is None:
            dout = torch.zeros_like(tape.x)
        if not ctx.frozen:
            # the user may have dropped p.grad (zero_grad(set_to_none=True)) -> overwrite semantics
            if eng._params()[tape.plan.first][1].grad is None:
                eng.grad_live = False
        need_x, need_t = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        dx, dt = eng.backward(tape, dout, list(dzs) if ctx.nz else None, need_x, need_t, ctx.frozen)
        return None, None, dx, dt, None, None, None, None


def sit_apply(model, x, t, y, inference=True):
    """Builds an autograd graph when gradients are enabled and any parameter is trainable, x.requires_grad or t.requires_grad;
    x.grad / t.grad come back in the caller's dtype and shape (the casts below are torch's, in front of the Function).  With an
    input that requires grad and NO trainable parameter the backward is the frozen-weight one (Engine.backward)."""
    ops.require_cuda(x, "x")
    eng = model.engine()
    drop = None
    if model.class_dropout_prob > 0:
        if model.force_drop_mask is not None:
            drop = model.force_drop_mask
        elif model.training:  # LabelEmbedder.token_drop (sit.py:84-93): device RNG draw
            drop = torch.rand(y.shape[0], device=y.device) < model.class_dropout_prob
    need_grad, frozen, plan = False, False, None
    if torch.is_grad_enabled():
        sig = eng.signature()
        frozen = not any(sig)
        need_grad = (not frozen) or x.requires_grad or t.requires_grad
    if need_grad:
        plan = eng.plan_for(x.requires_grad, t.requires_grad, sig)
    if need_grad and (x.requires_grad or t.requires_grad):
        if frozen and eng.reducer is not None:
            raise RuntimeError(FROZEN_WITH_REDUCER)
        if x.requires_grad and x.dtype != torch.float32:
            x = x.float()
        if t.requires_grad:
            t = t.reshape(-1)
            if t.dtype != torch.float32:
                t = t.float()
    if not need_grad:
        out, zs, _ = eng.forward(x, t, y, inference, False, drop)
        return out, zs
    if not frozen and (not hasattr(model, "_anchor") or model._anchor.device != x.device):
        model._anchor = torch.zeros(1, device=x.device, requires_grad=True)
    res = _SiTFunction.apply(None if frozen else model._anchor, model, x, t, y, inference, drop, plan)
    out, zs = res[0], (list(res[1:]) if len(res) > 1 else None)
    if inference:
        zs = None
    elif zs is None:
        zs = []
    return out, zs
