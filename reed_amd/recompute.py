"""The recompute plan: which blocks keep a checkpoint instead of their activations (host arithmetic only; Engine executes it).

A block that saves (freeze.py: plan.save) holds, per token and channel, eight operand-type arrays (h, qkv, o, u, h2, a1, y1, y2: 16
element-widths of D at mlp_ratio 4) and two fp32 residuals (xmid, and xout = the next block's input) from its forward until its
backward: 40 bytes in the 16-bit builds.  With SiT.recompute set, the N lowest-indexed blocks that have a backward — the ones whose
activations live longest — keep instead
  * their input x (fp32): the array the block below wrote as its xout, or the patch embedder's tokens — shared, not copied;
  * their y2 (operand type): the MLP gate's backward reads it, the LayerNorm backward of the block above reads it in its fused pass
    (Engine._ln_bwd), and with it the rebuild never runs fc2, a third of a block's forward GEMM work;
6 bytes, and the backward rebuilds the rest from x right before it runs the block, with the forward's own launches on the same
arguments: ln_modulate_fwd, qkv, (qk_norm_fwd,) attention_fwd, proj with the gate + residual epilogue (xmid, y1), ln_modulate_fwd,
fc1 with the epilogue the tape recorded (act_grad).  The blocks have no RNG, the 16-bit weight copies do not change between a step's
forward and its backward and the kernels are deterministic: the rebuilt arrays have the saved ones' bits, so every gradient keeps its
bits.  At most one block's rebuilt set is alive at a time; it is released where a saved record is.

The tape records what each block kept: changing SiT.recompute between a forward and its backward does nothing to that backward.
saved_activation_bytes is the closed form of what the tape of one forward holds, tensor by tensor.
"""
import operator

ALL = "all"


def normalize(value):
    """SiT.recompute -> 0 (off: None, False, 0), "all" (True, "all") or a positive int N.  Anything else raises."""
    if value is None or value is False:
        return 0
    if value is True:
        return ALL
    if isinstance(value, str):
        if value == ALL:
            return ALL
        raise ValueError(f"recompute={value!r}: 0, a number of blocks, True or 'all'")
    try:
        n = operator.index(value)
    except TypeError:
        raise ValueError(f"recompute={value!r}: 0, a number of blocks, True or 'all' (not a {type(value).__name__})") from None
    if n < 0:
        raise ValueError(f"recompute={value!r}: a number of blocks cannot be negative")
    return n


def recomputed_blocks(value, save):
    """[bool per block]: block i keeps a checkpoint and is rebuilt in the backward.  save[i]: block i has a backward (its forward
    saves; every block without a plan, FreezePlan.save with one): the blocks below a truncated plan's k save nothing already and do
    not count.  N above the number of blocks with a backward means all of them."""
    n = normalize(value)
    have = sum(1 for s in save if s)
    n = have if n == ALL else min(n, have)
    out, left = [], n
    for s in save:
        on = bool(s) and left > 0
        left -= on
        out.append(on)
    return out


def parse_flag(text):
    """--recompute-blocks {N,all} (argparse type)."""
    import argparse
    if text == ALL:
        return ALL
    try:
        return normalize(int(text))
    except ValueError:
        raise argparse.ArgumentTypeError(f"{text!r}: a number of blocks >= 0, or 'all'") from None


def max_tokens(widest, hb, T=1, ada_rows=0):
    """The largest token count M = B T of a forward that builds a graph, from the kernels' index arithmetic.  With recomputation a
    local batch several times today's fits in memory, so the range matters.  Read off the launchers and kernels of csrc/: the row
    kernels, the attention kernels, the GEMM epilogues and the forward / input-gradient GEMMs form row offsets in 64 bits (a buffer
    window per tile, leading dimensions below 2^20) and take M as an int; the narrowest range is the weight-gradient GEMMs' of the
    16-bit builds (TN layout: gemm_tn.hip stage_tr, gemm.hip / gemm256.hip / gemm256w.hip with a transposed operand), which address
    their token-major operands [M, width] through one buffer window from the array's start with a 32-bit BYTE offset: M * width * 2
    must stay below 2^31 for the widest such operand (`widest` elements per token: qkv's 3 D, the MLP's hidden width, a
    projector's).  Next comes the gate + residual epilogue's 32-bit byte offset into the modulation array [B, ada_rows]
    (gemm_common.hpp): B * ada_rows * 2 below 2^31, the narrower of the two only for a deep model on very few tokens per image.
    None of those launchers checks either; Engine._forward does.
    This is a conservative reading, not a measured limit: the offsets are formed as `(int)(... * 2)` and as running int sums
    (kbase + kstep), the hardware takes a buffer offset as an unsigned 32-bit value against num_records (make_rsrc clamps it to
    2^32 - 1), and a wrapped int keeps its bit pattern — so the kernels plausibly work up to 2^32 bytes, twice this bound.  But
    signed overflow of the running sums is undefined in C++, nothing has been run past 2^31, and a wrong answer there would be silent
    (reads beyond the window return zeros): the engine refuses where the arithmetic as written stops being defined.
    The fp32-operand build forms 64-bit element indices in what was read for this (gemm_f32.hip loads and epilogues,
    attention_f32.hip, norm.hip, qknorm.hip, embed.hip, lora.hip): there only the int M holds, less the 256-row tile the launchers
    round up by; the loss and sampler kernels, which never see a token-major activation, were not read."""
    if hb == 4:
        return 2 ** 31 - 257
    n = (2 ** 31 - 1) // (widest * hb)
    if ada_rows:
        n = min(n, T * ((2 ** 31 - 1) // (ada_rows * hb)))
    return n


# the operand-type arrays of a saved block in units of M elements, as (multiples of D, multiples of the MLP width)
SAVED_OPERAND_ARRAYS = {"h": (1, 0), "qkv": (3, 0), "o": (1, 0), "u": (0, 1), "h2": (1, 0), "a1": (0, 1), "y1": (1, 0), "y2": (1, 0)}


def block_bytes(M, D, Hm, H, hb, qk_norm=False, recomputed=False):
    """Bytes one block's record holds beside its input x (the residual shared with the block below): M = tokens, hb = bytes per
    operand element.  A saved block: the eight operand arrays, xmid, the four row statistics, lse [B, H, T] and, with qk_norm, the
    normalised qkv and its row statistics [M, 2, H, 2]; a recomputed one: y2."""
    if recomputed:
        return M * D * hb
    n = sum(d * D + h * Hm for d, h in SAVED_OPERAND_ARRAYS.values()) * M * hb      # h qkv o u h2 a1 y1 y2
    n += M * D * 4                                                                   # xmid
    n += 4 * M * 4 + M * H * 4                                                       # mean1 rstd1 mean2 rstd2, lse
    if qk_norm:
        n += M * 3 * D * hb + M * 2 * H * 2 * 4                                      # qkv_a, qstats
    return n


def saved_activation_bytes(B, T, D, Hm, H, depth, hb, save, recomputed, in_channels, input_size, ada_rows, qk_norm=False,
                           projectors=()):
    """Bytes the tape of one forward at batch B holds (Engine._forward with need_grad), every distinct tensor once:
      * the inputs x [B, C, HW, HW] and t [B] (fp32) and the embedders' records: the sinusoid [B, 256], the timestep MLP's t1p and
        t1, silu(c) [B, D] and the modulation [B, ada_rows] in the operand type, c [B, D] fp32, the effective labels [B] int64;
      * the residual stream: the input of every block with a record and the last block's output, fp32 [M, D] each — depth - k + 1
        arrays, a block's input being the array the block below wrote;
      * the blocks (block_bytes);
      * the final layer's row statistics;
      * projectors: (rows, width) of each projector with a record — its input [rows, D] and four [rows, width] arrays.
    save / recomputed: per block, as FreezePlan.save and recomputed_blocks give them."""
    M = B * T
    n = B * in_channels * input_size * input_size * 4 + B * 4
    n += B * 256 * hb + 3 * B * D * hb + B * ada_rows * hb + B * D * 4 + B * 8
    n += (sum(1 for s in save if s) + 1) * M * D * 4
    for s, r in zip(save, recomputed):
        if s:
            n += block_bytes(M, D, Hm, H, hb, qk_norm, r)
    n += 2 * M * 4
    for rows, width in projectors:
        n += rows * D * hb + 4 * rows * width * hb
    return n
