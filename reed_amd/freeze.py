"""The freeze plan: which backward launches a partly frozen SiT needs (host arithmetic only; Engine executes it).

torch's idiom for fine-tuning part of a model is p.requires_grad_(False) on the rest.  The engine reads every parameter's flag per
forward as one tuple (the signature), and plans once per signature:
  * a launch whose outputs are all gradients of frozen parameters is skipped; a launch with mixed outputs (a frozen weight with a
    trainable bias, one block's rows of the stacked adaLN GEMM) runs as it does in the fully trainable model, its frozen outputs
    landing in the gradient arena where nothing reads them (p.grad stays None, the optimiser walks the trainable ranges only);
  * the grouped weight-gradient launch serves a block whose four linears all need theirs, the per-GEMM launches the rest;
  * the adapters of an adapted linear (lora_A / lora_B) take a launch of their own off the linear's (dy, x) pair, beside the base
    weight's launch or instead of it; they count like the linear itself for stages, truncation and what the forward saves;
  * truncation: with x_embedder, t_embedder, y_embedder and every block below k frozen and no input requiring grad, nothing below
    block k consumes the activation-gradient chain — blocks < k run no backward and save nothing in the forward, the conditioning
    tail is skipped, block k stops at the stage that completes its own gradients, and a projector tap forms its contribution to
    the trunk's dx only where a block that runs consumes it.
With every parameter trainable (mode "all") and with none (mode "none": the frozen-weight backward behind an input that requires
grad) the plan is the launch sequence those two cases always had.
"""
import fnmatch

LINEARS = ("mlp.fc2", "mlp.fc1", "attn.proj", "attn.qkv")    # in backward order
# the stage of a block's backward that completes a gradient (Engine._backward_block runs stages 1 .. stage[i] of block i):
#   1 dy2 -> fc2 | 2 da1 -> fc1 | 3 LN2 backward + gate: dy1 -> proj | 4 attention (+ qk-norm) backward: dqkv -> qkv, q/k norm
#   5 LN1 backward and the block's modulation gradients (its adaLN rows; dx for the block below)
STAGE_OF = {"mlp.fc2": 1, "mlp.fc1": 2, "attn.proj": 3, "attn.qkv": 4}
PROJ_LAYERS = (4, 2, 0)                                       # in backward order


class FreezePlan:
    def __init__(self, depth, tap_depth, trainable, qk_norm=False, need_x=False, need_t=False, all_names=None):
        """trainable: the names of the parameters that require grad; tap_depth[j]: projector j reads the output of block
        tap_depth[j] - 1; all_names: every parameter name but pos_embed (mode "all" is decided against it)."""
        tr = frozenset(trainable) - {"pos_embed"}
        self.depth, self.need_x, self.need_t = depth, bool(need_x), bool(need_t)
        self.trainable = tr
        self.any = bool(tr)
        if all_names is not None and tr >= frozenset(all_names) - {"pos_embed"}:
            self.mode = "all"
        else:
            self.mode = "partial" if tr else "none"

        def on(prefix):
            return prefix + ".weight" in tr or prefix + ".bias" in tr

        def lo(prefix):   # the adapters of an adapted linear (reed_amd/lora.py): their own launch off the linear's (dy, x) pair
            return prefix + ".lora_A" in tr or prefix + ".lora_B" in tr

        # what each launch would write
        self.lin = [{n: on(f"blocks.{i}.{n}") for n in LINEARS} for i in range(depth)]
        self.lora = [{n: lo(f"blocks.{i}.{n}") for n in LINEARS} for i in range(depth)]
        self.qknorm = [bool(qk_norm) and (on(f"blocks.{i}.attn.q_norm") or on(f"blocks.{i}.attn.k_norm")) for i in range(depth)]
        self.ada = [on(f"blocks.{i}.adaLN_modulation.1") for i in range(depth)] + [on("final_layer.adaLN_modulation.1")]
        self.any_ada = any(self.ada)
        self.group = [all(d.values()) for d in self.lin]
        self.final_w = on("final_layer.linear")
        self.x_emb = on("x_embedder.proj")
        self.t0, self.t2 = on("t_embedder.mlp.0"), on("t_embedder.mlp.2")
        self.label = "y_embedder.embedding_table.weight" in tr
        self.proj_w = [{k: on(f"projectors.{j}.{k}") for k in PROJ_LAYERS} for j in range(len(tap_depth))]
        block_on = [any(self.lin[i].values()) or any(self.lora[i].values()) or self.qknorm[i] or self.ada[i] for i in range(depth)]
        # the chain runs to the bottom for the patch embedder or dL/dx; the conditioning tail (which reads every block's
        # modulation gradients) for the timestep MLP, the label table or dL/dt
        bottom = self.x_emb or self.need_x
        self.cond = self.t0 or self.t2 or self.label or self.need_t or bottom or self.mode != "partial"
        self.trunc = not self.cond
        if not self.trunc:
            self.k = 0
            self.stage = [5] * depth
        else:
            self.k = next((i for i in range(depth) if block_on[i]), depth)
            self.stage = [0] * self.k + [5] * (depth - self.k)
            if self.k < depth:
                i = self.k
                s = max([STAGE_OF[n] for n in LINEARS if self.lin[i][n] or self.lora[i][n]] +
                        [4 if self.qknorm[i] else 0, 5 if self.ada[i] else 0])
                self.stage[i] = s
        self.save = [s > 0 for s in self.stage]
        # the final layer: its row kernel for its linear's gradients or the chain; its LayerNorm backward for the chain or its adaLN rows
        self.final_ln = (not self.trunc) or self.k < depth or self.ada[depth]
        self.final_run = self.final_ln or self.final_w
        # modulation gradients are gathered (dmod) for the conditioning tail or trainable adaLN rows; block i's reduce feeds them
        self.dmod = self.cond or self.any_ada
        self.mod_reduce = [self.cond or (self.ada[i] and (i == depth or self.stage[i] == 5)) for i in range(depth + 1)]
        # projector j: its chain runs down to the lowest layer with a trainable parameter, or through, into the trunk's dx, where
        # the block below the tap runs
        self.proj = []
        for j, dj in enumerate(tap_depth):
            dx = (not self.trunc) or (dj - 1 >= self.k and self.stage[dj - 1] > 0)
            need = [k for k in PROJ_LAYERS if self.proj_w[j][k]]
            stop = -1 if dx else (min(need) if need else None)     # -1: through layer 0's input gradient
            self.proj.append({"run": stop is not None, "dx": dx, "stop": stop, "w": self.proj_w[j], "tap": dj})
        self.any_proj_w = any(any(w.values()) for w in self.proj_w)

    def launches(self):
        """Names of the parameter-gradient launches the backward issues, in order (the activation-gradient chain between them is
        given by stage / final_ln / cond / proj).  `block{i}.wgrad` lists the linears; the engine groups them into one launch
        where group[i] holds and the device fits the grouped kernel."""
        out = []
        if self.final_w and self.final_run:
            out.append("final.smallk_wgrad")
        taps = {}
        for j, pj in enumerate(self.proj):
            taps.setdefault(pj["tap"], []).append(j)

        def proj(j):
            pj = self.proj[j]
            if pj["run"]:
                for k in PROJ_LAYERS:
                    if pj["w"][k] and (pj["stop"] == -1 or k >= pj["stop"]):
                        out.append(f"proj{j}.wgrad.{k}")

        for i in reversed(range(self.k, self.depth)):
            for j in taps.get(i + 1, ()):
                proj(j)
            for n in LINEARS:
                if self.lin[i][n] and STAGE_OF[n] <= self.stage[i]:
                    out.append(f"block{i}.wgrad.{n}")
                if self.lora[i][n] and STAGE_OF[n] <= self.stage[i]:
                    out.append(f"block{i}.lora.{n}")
            if self.qknorm[i] and self.stage[i] >= 4:
                out.append(f"block{i}.qknorm_rowsum")
        for dj in sorted(taps, reverse=True):
            if dj <= self.k:
                for j in taps[dj]:
                    proj(j)
        if self.any_ada:
            out.append("ada.wgrad")
        if self.cond:
            if self.label:
                out.append("label_scatter")
            if self.t2:
                out.append("t.wgrad.2")
            if self.t0:
                out.append("t.wgrad.0")
            if self.x_emb:
                out.append("x.smallk_wgrad")
        return out


def trainable_ranges(layout, trainable):
    """Sorted, merged [begin, end) arena ranges of the trainable parameters, each parameter with the padding behind it (segments
    are 8-aligned, the trained part of the arena 64-aligned: every bound is a multiple of 4; the padding holds zeros that never
    receive a gradient).  Adjacent parameters merge, so a handful of ranges covers the usual freeze sets."""
    names = [n for n in layout.seg if n != "pos_embed"]
    out = []
    for n, nxt in zip(names, names[1:] + [None]):
        if n not in trainable:
            continue
        b = layout.seg[n][0]
        e = layout.seg[nxt][0] if nxt is not None else layout.n_train
        if out and out[-1][1] == b:
            out[-1][1] = e
        else:
            out.append([b, e])
    return [(b, e) for b, e in out]


def select_parameters(names, freeze=None, train_only=None):
    """The trainable subset of `names` for --freeze PATTERN [...] / --train-only PATTERN [...] (fnmatch on parameter names, one
    of the two); a pattern that matches no parameter is an error."""
    if freeze and train_only:
        raise ValueError("--freeze and --train-only are mutually exclusive")
    names = list(names)
    pats = freeze or train_only
    if not pats:
        return set(names)
    hit = set()
    for pat in pats:
        m = fnmatch.filter(names, pat)
        if not m:
            raise ValueError(f"pattern {pat!r} matches no parameter (names look like {names[0]!r}, {names[-1]!r})")
        hit.update(m)
    return set(names) - hit if freeze else hit
