"""RAFT orchestrator (reference: core/raft.py:13-108): same constructor, same
``forward(images, poses, intrinsics, scale=None, do_report=False)``, same state_dict keys
(fnet.*, cnet.*, update_block.*; a ``module.`` prefix from DataParallel checkpoints is accepted).

Test-mode forward = both encoders on the channels-last HIP engine (encoder_hip.py: producer / consumer convolutions, csrc/enc_pc.hip;
``encoder_backend="miopen"`` selects the PyTorch-ROCm modules), then per cascade stage one fused cost-volume build (view-mean folded,
level-0 rows) and T x 5 HIP kernels (lookup incl. the previous iteration's disparity update, corr2, z|r, q, fused delta head); see
DESIGN.md for the data layout.  Differences from the
reference that a caller can observe, all deliberate (SURVEY.md §8(a) "quirks"):
  * `images` and `poses` are NOT mutated in place (reference: raft.py:35,40-41);
  * `scale` may be a float or a tensor on any device (reference: raft.py:108 calls scale.cuda());
  * computation is fp32 end to end by default (``precision="fp32"``); the reference's GPU path runs
    encoders + GRU under fp16 autocast (raft.py:9,55), selectable with ``precision="amp"`` for the
    encoders only.  ``gru_precision`` picks the arithmetic of the update block's 3x3 convolutions: "auto" (default: the first
    AUTO_INPUTS forwards of a set of weights walk the candidates of AUTO_FORMS, cheapest first - each input runs in the last form,
    "s16", and in the current candidate; a candidate further than AUTO_TOL from "s16" is demoted to the next form, which is tested on
    the same input, and "s16" ends the walk - see __init__),
    "s16f8" (split-f16 operands, x*w = xh*wh + (xh*wl + xl*wh) into one fp32 accumulator with the main term on the f16
    matrix instruction and the two 2^-11 correction terms on the block-scaled fp8 one - 4e-6 relative L1 from fp32 end to end,
    csrc/conv_s16.hip), "s16" (all three terms in f16: fp32-class, 2e-7), "f16x3" (round-1 kernels: two fp32 accumulators) or
    "fp32" (exact v_mfma_f32_16x16x4_f32).
Multi-GPU: ``view_group`` = a torch.distributed process group (one rank per GPU, RCCL over xGMI).  ``shard="slab"``
(default): source views are sharded for the encoders (all-gather of the feature maps), image rows are sharded for the cost
volume and the GRU loop with a 7-row halo exchange per iteration (slab.py) - strong scaling of one depth map;
``shard="views"``: views sharded, view-sum volume all-reduced once per stage, GRU replicated (the simpler fallback, also
used when a slab would be thinner than the halo)."""
import torch
import torch.nn as nn

from . import dist as cdist
from . import ops
from .corr import CorrBlock, fmaps_to_nhwc, report
from .extractor import BasicEncoder
from .projective import pij_matrices, scaled_cameras
from .update import UpdateBlock


class SaturationError(RuntimeError):
    """A split-f16 kernel clamped an operand.  A RuntimeError subclass of its own so that callers which clean up after
    THIS condition (``inference``: the depth maps written before the flag could be read) do not do so for unrelated RuntimeErrors -
    an out-of-memory error, a loader failure, a shape error."""


class RAFT(nn.Module):
    def __init__(self, cascade=[(64, 64, 8), (-1, 320, 8)], encoder_type="HR", dim_fmap=64, dim_net=64, dim_inp=64,
                 test_mode=False, precision="fp32", view_group=None, gru_precision="auto", encoder_backend="hip", shard="slab",
                 enc_precision="auto", cost_precision="auto", train_backend="torch"):
        super().__init__()
        self.cascade = [tuple(c) for c in cascade]
        self.encoder_type = encoder_type
        self.dim_fmap, self.dim_net, self.dim_inp = dim_fmap, dim_net, dim_inp
        self.test_mode = test_mode
        # train_backend: the lookup and the loss upsample of the training row (train.py): "torch" (grid_sample / F.interpolate) or "hip"
        # (csrc/train_ops.hip: atomics-free adjoints, runs under torch.use_deterministic_algorithms)
        if train_backend not in ("torch", "hip"):
            raise ValueError(f"RAFT: unknown train_backend {train_backend!r}")
        self.train_backend = train_backend
        self.precision = precision
        self.view_group = view_group
        self.shard = shard
        self.fnet = BasicEncoder(output_dim=dim_fmap, norm_fn="instance", type=encoder_type)
        self.cnet = BasicEncoder(output_dim=dim_net + dim_inp, norm_fn="none", type=encoder_type)
        self.update_block = UpdateBlock(cascade=self.cascade, dim_net=dim_net, dim_inp=dim_inp)
        if gru_precision not in ("auto", "s16f6", "s16f8", "s16", "f16x3", "fp32"):
            raise ValueError(f"RAFT: unknown gru_precision {gru_precision!r}")
        self.gru_precision = gru_precision
        # enc_precision (round 6): arithmetic of the encoders' producer / consumer convolutions (csrc/enc_pc.hip).  "f16x3": three f16 MFMA
        # terms per product (fp32-class; rounds 2-5); "f6": the two correction terms on the FP6 (e2m3, block-scaled) form of
        # v_mfma_scale_f32_32x32x64_f8f6f4 - half the matrix cycles, features 4e-5 from the f16 form; "auto" (default): part of the
        # gru_precision="auto" calibration walk (AUTO_FORMS: a "+e6" suffix = encoders in the FP6 form) and "f16x3" whenever gru_precision is pinned.
        if enc_precision not in ("auto", "f16x3", "f6"):
            raise ValueError(f"RAFT: unknown enc_precision {enc_precision!r}")
        self.enc_precision = enc_precision
        self._enc_f6 = enc_precision == "f6"
        # cost_precision (round 6): the dots of the epipolar-line-tile cost volume (csrc/cost_lines.hip).  "x3": three split-f16 terms (fp32-class);
        # "x2": the source texels' lo planes are not read (source features as f16) - half the fragment bytes that bound the tile kernel,
        # 1.2e-5 on the volume, ~5e-6 on the disparity; "auto" (default): a "+c2" suffix of the calibration walk's forms, "x3" with a pinned gru_precision.
        if cost_precision not in ("auto", "x3", "x2"):
            raise ValueError(f"RAFT: unknown cost_precision {cost_precision!r}")
        self.cost_precision = cost_precision
        self._cost_x2 = cost_precision == "x2"
        self.update_block.conv_mode = "s16" if gru_precision in ("s16f6", "s16f8", "auto") else gru_precision
        self._set_form(gru_precision if gru_precision != "auto" else self._auto_forms()[0])
        # "auto" (default): the fp8-correction form keeps ~15 product bits in the correction terms; how much of that reaches the depth
        # depends on how the update block's weights condition the 32-iteration recurrence (tests/test_determinism_gpu.py: 22-38 x the
        # all-f16 form's distance from exact fp32 - 3e-6 on the golden weights, 3e-4 with the conv weights doubled and heavy-tailed).
        # So the FIRST AUTO_INPUTS (3) test-mode forwards of a set of weights are calibration forwards, each on its own input (conditioning
        # also depends on the scene, VERDICT r4 "weak" 1c).  They walk a LIST of candidates (_auto_forms: AUTO_FORMS, cheapest first; the last
        # one, "s16", is the fp32-class reference): every calibration input runs in the last form and in the current candidate; if the two
        # disparities differ by more than AUTO_TOL relative L1 (or AUTO_MAX_TOL of the largest disparity at any single pixel) the candidate
        # is demoted to the next form (with a warning), which is tested on the same input; reaching the last form ends the walk.  The
        # candidate that stands after the last calibration input is kept.  The extra forwards buy the cheaper forms' speed wherever they are
        # safe, and the fp32-class margin wherever they are not.  Callers who need a decision that does not depend on which inputs come
        # first pin gru_precision explicitly.  A further form exists - "s16f6", the correction terms on the FP6 form of the same instruction
        # (half its matrix-pipe passes again; one E8M0 scale per 16-channel block) - see AUTO_FORMS for why it is not a default candidate.
        self.auto_choice = None                   # None until decided; then the form that stands (one of _auto_forms())
        self.auto_error = None                    # the worst relative L1 from the last form among the comparisons that passed (a walk
                                                  # that ended at the last form: the last demoted candidate's)
        self._auto_sig = None
        self._auto_left = 0                       # calibration forwards still to run for the current set of weights
        self.encoder_backend = encoder_backend      # "hip": channels-last engine (csrc/enc_conv.hip); "miopen": PyTorch-ROCm convs
        self._engines = None
        self._src_buf = {}
        self.last_timings = None
        # What to do when a split-f16 kernel had to clamp an operand (ops.check_overflow; cer_mvs.h "Saturation is never silent"):
        #   "lazy"  (default) the flag is read at the START of the next forward (no extra synchronisation) and by check_overflow();
        #           a hit raises there;  "raise": read at the end of every forward (one device->host read);  "fallback": as "raise",
        #           but the forward is repeated with the wide-range arithmetic (gru_precision "f16x3", fp32 cost-volume walk);
        #   "ignore": never read.
        self.overflow_policy = "lazy"
        # packed encoder weights are a cache of the parameters: drop them whenever parameters are (re)loaded - through this
        # module, a wrapper (nn.DataParallel(model).load_state_dict, as the reference's inference.py does) or a submodule
        # (the hooks hold a weak reference: a deep copy's hooks still point at the ORIGINAL model, which is why the packs are also
        # validated against the parameters' storage + version counters on every forward, ``_params_sig``)
        import weakref
        me = weakref.ref(self)
        for m in (self, self.fnet, self.cnet):
            m.register_load_state_dict_post_hook(lambda module, incompatible, me=me: me() is not None and me()._drop_engines())
        self._sig = None

    def _drop_engines(self):
        self._engines = None

    def _set_form(self, form):
        """arithmetic form of a forward: a gru_precision name, optionally "+e6" (encoders in the FP6-correction form; honoured with enc_precision="auto") and / or "+c2" (two-term cost-volume dots; cost_precision="auto")"""
        g, *sfx = form.split("+")
        self.update_block.corr_fp8 = self._CORR_FORM.get(g, False)
        self._enc_f6 = self.enc_precision == "f6" or (self.enc_precision == "auto" and "e6" in sfx)
        self._cost_x2 = self.cost_precision == "x2" or (self.cost_precision == "auto" and "c2" in sfx)

    def _get_engines(self, dev):
        from .encoder_hip import HipEncoder
        if self._engines is None or self._engines[0] != dev:
            self._engines = (dev, HipEncoder(self.fnet, dev), HipEncoder(self.cnet, dev))
        self._engines[1].f6 = self._engines[2].f6 = bool(self._enc_f6)
        return self._engines

    def _params_sig(self):
        """Identity + in-place version of every parameter: packed weights are a cache of these (optimizer steps, copy_, deepcopy)."""
        return tuple((p_.data_ptr(), p_._version) for p_ in self.parameters())

    def _validate_packs(self):
        sig = self._params_sig()
        if sig != self._sig:
            if self._sig is not None:
                self._engines = None
                self.update_block.refresh_weights()
            self._sig = sig

    _OVERFLOW_WHAT = {1: "cost-volume feature rows beyond +-1023 (after the reference's /8)", 2: "hidden map of the delta head beyond 4094",
                      4: "a ReLU-class activation of the update block (inp, corr features) beyond 4094",
                      8: "a disparity of the update loop beyond +-5.1175 (its generated 7x7 difference features clamp at 10.235)"}

    def check_overflow(self, device=None, raise_error=True):
        """Read (and clear) the sticky saturation flag of the split-f16 kernels; returns the bits, raises RuntimeError on a hit."""
        device = device if device is not None else next(self.parameters()).device
        bits = ops.check_overflow(device)
        if bits and raise_error:
            self._raise_overflow(bits)
        return bits

    def _raise_overflow(self, bits):
        what = "; ".join(v for k, v in self._OVERFLOW_WHAT.items() if bits & k)
        raise SaturationError(f"cer-mvs_amd: a split-f16 kernel saturated an operand ({what}): the result of that forward is not fp32-class. "
                           "Use RAFT(..., gru_precision='f16x3') / _lib.load().cer_cost_build_algo(1), or overflow_policy='fallback'.  "
                           "(f16x3 carries activations at scale 1: its own clamp, at 65504, is 16 x further out and is NOT reported.  A disparity "
                           "beyond +-5.1175 has no arithmetic remedy: it is reported in every form, and such a depth range is a wrong input.)")

    def refresh_weights(self):
        """Call after mutating parameters in place: drops every packed copy (encoder engines, update-block packs)."""
        self._engines = None
        self.update_block.refresh_weights()

    def stages(self):
        """(D, incre, T) per cascade stage (reference: core/raft.py:76-81)."""
        out = []
        for nIncre, incre, nIters in self.cascade:
            if nIncre == -1:
                nIncre = (2 * self.update_block.radius + 1) * 2 ** (self.update_block.num_levels - 1)
            out.append((nIncre, 0.0025 / incre, nIters))
        return out

    # ---------------------------------------------------------------- encoders (HIP engine by default; encoder_backend="miopen": PyTorch-ROCm)
    def _apply(self, fn, *a, **k):
        self._engines = None            # weights moved / cast: repack on next use
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, strict=True, **kw):
        """Accepts DataParallel-style ``module.``-prefixed checkpoints (reference: inference.py:31-35)."""
        if state_dict and all(k.startswith("module.") for k in state_dict):
            state_dict = {k[7:]: v for k, v in state_dict.items()}
        self._engines = None
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def encode(self, images, views, raw=False, parts="all"):
        """images [1,N,3,H,W] in [-1,1] (``raw``: 0..255, normalised on the fly, core/raft.py:40-41); ``views`` = source-view
        indices this rank owns -> (net [P,64], inp [P,64], reference features [P,C], source features [len(views),(h+4)*(w+4),C]);
        features are channels-last, scaled by 1/8, source maps with a 2-texel zero border.
        ``parts``: "all", or "src" (source features only: (None, None, None, f2)) / "ref" (context + reference features:
        (net, inp, f1, None)) - the sharded forward encodes its source views first, starts their all-gather, and encodes the
        reference view while the collective is in flight."""
        views = [] if parts == "ref" else list(views)
        ref = parts != "src"
        if not ref and not views:
            return None, None, None, None
        idx = ([0] if ref else []) + views
        stack = images[0] if idx == list(range(images.shape[1])) else images[0, idx]      # (no gather copy when every view is local)
        if self._hip_encoders():
            dev = images.device
            _, eng_f, eng_c = self._get_engines(dev)
            net, inp, h, w = None, None, images.shape[-2] // 4, images.shape[-1] // 4
            if ref:
                net, inp, h, w = eng_c.context(images[0, :1], raw=raw)
            buf = self._source_buffer((len(views), h, w, str(dev)), lambda: torch.zeros(
                len(views), (h + 4) * (w + 4), self.dim_fmap, device=dev, dtype=torch.float32)) if views else None
            f1, src, _, _ = eng_f.features(stack, n_ref=int(ref), border=2, scale=0.125, src_out=buf, raw=raw)
            return net, inp, f1[0] if ref else None, src
        if raw:
            stack = stack.float() * (2 / 255.0) - 1
        with torch.autocast("cuda", dtype=torch.float16, enabled=self.precision == "amp"):
            ctx = self.cnet(stack[None, :1])[0, 0].float() if ref else None      # [128,h,w]
            fm = self.fnet(stack).float()                                      # [n,C,h,w] (instance norm is per image)
        if not ref:
            return None, None, None, fmaps_to_nhwc(fm, border=2)
        net = torch.tanh(ctx[: self.dim_net])
        inp = torch.relu(ctx[self.dim_net:])
        f2 = fmaps_to_nhwc(fm[1:], border=2) if views else None
        return ops.nchw_to_nhwc(net.contiguous()), ops.nchw_to_nhwc(inp.contiguous()), fmaps_to_nhwc(fm[:1])[0], f2

    def _hip_encoders(self):
        """The HIP encoder engines (encoder_hip.py) serve this model; otherwise the PyTorch-ROCm modules do."""
        return self.encoder_backend == "hip" and self.precision == "fp32" and self.encoder_type == "HR"

    def _source_buffer(self, key, make):
        """The persistent buffer the feature head writes the source views into: its border texels are written once (zeros, by ``make``)
        and never touched again.  One live entry: a new key (view count, feature grid, device, layout) replaces it."""
        if key not in self._src_buf:
            self._src_buf = {key: make()}
        return self._src_buf[key]

    def _encode_direct_split(self, images, V, h, w):
        """encode() whose feature head writes the cost volume's split-f16 operand planes directly -> (net, inp, (f1s, f2s, slots))."""
        dev = images.device
        _, eng_f, eng_c = self._get_engines(dev)
        net, inp, _, _ = eng_c.context(images[0, :1], raw=True)
        f2s, slots = self._source_buffer(("split", V, h, w, str(dev)), lambda: (
            torch.zeros(V, (h + 4) * (w + 4), 128, device=dev, dtype=torch.float16), torch.arange(V, device=dev, dtype=torch.int32)))
        f1s = torch.empty(h * w, 128, device=dev, dtype=torch.float16)
        eng_f.features_split(images[0], f1s, f2s, n_ref=1, border=2, scale=0.125, raw=True, flag=ops.overflow_flag(dev))
        return net, inp, (f1s, f2s, slots)

    # ---------------------------------------------------------------- forward
    def forward(self, images, poses, intrinsics, scale=None, do_report=False):
        if not images.is_cuda:
            raise RuntimeError("RAFT.forward: images must be a CUDA tensor (there is no CPU path)")
        if not self.test_mode:
            # training mode: the list of per-iteration predictions (core/raft.py:103,109), differentiable (train.py)
            from .train import forward_train
            return forward_train(self, images, poses, intrinsics, scale)
        if "mean" not in self.update_block.aggregation or len(self.update_block.aggregation) != 1:
            return self._forward_literal(images, poses, intrinsics, scale, do_report)
        dev = images.device
        if scale is None:
            raise AssertionError("scale is required in test mode (reference: core/raft.py:107)")
        batch, num, ch, ht, wd = images.shape
        if batch != 1:
            raise RuntimeError("RAFT.forward: batch must be 1 in test mode")
        return self._with_policy(dev, lambda: self._forward_fast(images, poses, intrinsics, scale, do_report),
                                 lambda: self._forward_calibrating(images, poses, intrinsics, scale, do_report))

    def _with_policy(self, dev, run, calibrate=None):
        """The overflow policy around one forward, shared by ``forward`` and ``forward_cached``.  ``run()``: the forward in the model's
        current arithmetic form; ``calibrate()``: the calibrating forward of gru_precision="auto" (None: the caller has made sure that no
        calibration is pending)."""
        pending = lambda: calibrate is not None and self.gru_precision == "auto" and self._auto_pending()
        if self.overflow_policy == "fallback" and self.view_group is not None:
            raise NotImplementedError("RAFT.overflow_policy='fallback' is not available with view_group (every rank would have to repeat "
                                      "the forward together): use 'lazy' or 'raise'")
        if self.overflow_policy == "lazy":
            bits = ops.overflow_poll(dev)              # what an EARLIER forward left (asynchronous snapshot: never blocks)
            if bits:
                self._raise_overflow(bits)
            if pending():
                return calibrate()
        elif self.overflow_policy in ("raise", "fallback") and self.view_group is None:
            if pending():
                calibrate()                            # (decides the form; the policy's own forward follows)
                self.check_overflow(dev, raise_error=False)
            out = run()
            bits = self.check_overflow(dev, raise_error=self.overflow_policy == "raise")
            if bits:                                   # fallback: repeat with the wide-range arithmetic
                from . import _lib as L
                mode, algo = self.update_block.conv_mode, L.load().cer_cost_build_algo(1 if bits & 1 else -1)
                self.update_block.conv_mode = "f16x3" if bits & 14 else mode
                try:
                    out = run()
                finally:
                    self.update_block.conv_mode = mode
                    L.load().cer_cost_build_algo(algo)
                ops.check_overflow(dev)
            return out
        if pending():
            return calibrate()
        return run()     # ("raise" with a view_group: handled at its end)

    _CORR_FORM = {"s16f6": 6, "s16f8": True, "s16": False}      # UpdateBlock.corr_fp8 of a split-f16 form
    # gru_precision="auto": candidates, cheapest first (the last one is the fp32-class reference).  "s16f6" is NOT among them by default: built and
    # measured in round 6 it costs the same time as "s16f8" - the chunk loop is not bound by the matrix pipe any more - and
    # sits 1.3 x further from fp32; a caller may put it in front (RAFT.AUTO_FORMS = ("s16f6", "s16f8", "s16")) or pin gru_precision="s16f6".
    # Round 6, second half: a "+e6" suffix puts the ENCODERS' correction terms on the FP6 form as well (csrc/enc_pc.hip; enc_precision="auto" only -
    # with the encoders pinned the suffixed candidates drop out, `_auto_forms`).  There it does pay (+ 3.8 % depth maps per second, same-box A/B,
    # profiles/r06_encoder_fp6_ab.txt; 1.2e-5 from the reference capture on the bench workload), so it IS the first default candidate.
    # "+c2": the cost volume's dots without the source texels' lo planes (csrc/cost_lines.hip, cost_precision="auto" only): + 5.6 % depth maps per second
    # on top (profiles/r06_cost_two_term_ab.txt), 1.23e-5 from the reference capture on the bench workload against 1.22e-5 without it.
    AUTO_FORMS = ("s16f8+e6+c2", "s16f8+e6", "s16f8", "s16")
    AUTO_TOL = 2.5e-5                             # a quarter of the 1e-4 parity bar
    AUTO_MAX_TOL = 1e-3                           # ... and no single pixel further apart than this fraction of the largest disparity
    AUTO_INPUTS = 3                               # inputs the decision rests on (the worst one counts)

    def _auto_forms(self):
        """the calibration walk's candidates for this model: AUTO_FORMS, without the "+e6" forms when the encoders' arithmetic is pinned"""
        ok = lambda f: ("e6" not in f.split("+") or self.enc_precision == "auto") and ("c2" not in f.split("+") or self.cost_precision == "auto")
        return tuple(f for f in self.AUTO_FORMS if ok(f))

    def _auto_pending(self):
        return self.update_block.conv_mode == "s16" and (self._auto_sig != self._params_sig() or self._auto_left > 0)

    def adopt_precision(self, other):
        """Take over another model's gru_precision="auto" decision instead of calibrating (the caller vouches that the weights are the
        same: DepthMapPipeline's replicas are deep copies of its first model).  Keeps the replicas of a pipeline on ONE arithmetic form -
        separate calibrations on different inputs could decide differently near the tolerance - and saves their calibration forwards.
        Returns True if a decision was adopted."""
        if (self.gru_precision != "auto" or other.gru_precision != "auto" or other.auto_choice is None or other._auto_pending()
                or self.update_block.conv_mode != other.update_block.conv_mode):
            return False
        self.update_block.corr_fp8, self._enc_f6, self._cost_x2 = other.update_block.corr_fp8, other._enc_f6, other._cost_x2
        self.auto_choice, self.auto_error = other.auto_choice, other.auto_error
        self._auto_sig, self._auto_left = self._params_sig(), 0
        return True

    def _forward_calibrating(self, images, poses, intrinsics, scale, do_report):
        """gru_precision="auto": this set of weights is still being calibrated - one step of the walk over ``_auto_forms()`` (AUTO_FORMS,
        cheapest first; the last form is the fp32-class reference).  The input runs in the last form and in the current candidate (the
        form that stood after the previous calibration input; the first form for new weights) and the two results are compared (relative
        L1 and largest single difference; all ranks of a view_group agree on the worst rank's figures).  A candidate outside the
        tolerances is demoted to the next form, which is tested on this same input; reaching the last form ends the walk for these
        weights.  A candidate that passes stands, and AUTO_INPUTS inputs are tested in all.  Returns the result of the form that stands
        after this input."""
        ub = self.update_block
        if self._auto_sig != self._params_sig():   # new weights: start over
            self._auto_left, self.auto_error, self.auto_choice = self.AUTO_INPUTS, 0.0, None
        forms = self._auto_forms()
        ref_form = forms[-1]
        self._set_form(ref_form)
        out16 = self._forward_fast(images, poses, intrinsics, scale, do_report).clone()
        self._auto_sig = self._params_sig()
        if ub.conv_mode != "s16":                  # (the weights did not fit a shared split-f16 scale: the forward fell back to f16x3 kernels)
            self._auto_left = 0
            return out16
        den = out16.abs().sum().clamp_min(1e-30)
        big = out16.abs().max().clamp_min(1e-30)
        cand = self.auto_choice if self.auto_choice in forms else forms[0]
        out, tried = out16, []
        while cand != ref_form:
            self._set_form(cand)
            outc = self._forward_fast(images, poses, intrinsics, scale, do_report)
            diff = (outc - out16).abs()
            err = float((diff.sum() / den).item())
            emax = float((diff.max() / big).item())
            if self.view_group is not None:
                err = cdist.max_float(err, self.view_group, images.device)
                emax = cdist.max_float(emax, self.view_group, images.device)
            tried.append((cand, err, emax))
            if err == err and emax == emax and err <= self.AUTO_TOL and emax <= self.AUTO_MAX_TOL:
                self.auto_error = max(self.auto_error or 0.0, err)
                out = outc
                break
            cand = forms[forms.index(cand) + 1]      # demoted: the next form is tested on this same input
        if cand == ref_form and tried:
            self.auto_error = tried[-1][1]
        ok = cand != ref_form
        self._auto_left = (self._auto_left - 1) if ok else 0
        self.auto_choice = cand
        self._set_form(cand)
        if any(e > self.AUTO_TOL or m > self.AUTO_MAX_TOL or e != e or m != m for _, e, m in tried):
            import warnings
            missed = "; ".join(f"{f}: {e:.2e} relative L1, largest single difference {m:.2e} of the largest disparity" for f, e, m in tried
                               if e > self.AUTO_TOL or m > self.AUTO_MAX_TOL or e != e or m != m)
            warnings.warn(f"cer-mvs_amd: gru_precision='auto': on one of this model's first {self.AUTO_INPUTS} inputs the distance from the all-f16 form "
                          f"('s16', fp32-class) was {missed} (tolerances {self.AUTO_TOL:.1e} / {self.AUTO_MAX_TOL:.1e}): keeping "
                          f"gru_precision={cand!r} for these weights")
        return out

    def _split_path(self, dev, V):
        """A single-GPU forward with V source views takes the direct-split path: every stage builds its volume on the epipolar-line
        tiles, so the feature head writes the cost volume's split-f16 operand planes itself (encoder_hip.features_split) - no fp32
        feature maps, no feat_split pass.  Otherwise the plain ``encode`` applies."""
        return bool(self.view_group is None and V >= 1 and self._hip_encoders()
                    and all(ops.on_line_tiles(self.dim_fmap, D_) for D_, _, _ in self.stages())
                    and self._get_engines(dev)[1].supports_split_head())

    def supports_cached(self, dev):
        """``forward_cached`` applies: a test-mode forward of this model takes the direct-split path (HIP "HR" encoders in fp32, every stage
        on the epipolar-line tiles, no view_group, view-mean aggregation), whatever the number of views, and its overflow policy does
        not need the fp32 walk (which reads fp32 source maps that a feature store does not keep)."""
        agg = self.update_block.aggregation
        if not self.test_mode or "mean" not in agg or len(agg) != 1 or self.overflow_policy == "fallback":
            return False
        return self._split_path(dev, 1)              # (the number of views does not enter beyond V >= 1)

    def _forward_fast(self, images, poses, intrinsics, scale, do_report):
        self._validate_packs()
        dev = images.device
        batch, num, ch, ht, wd = images.shape
        factor = 8 if self.encoder_type == "LR" else 4
        if self.view_group is not None and self.shard == "slab":
            from . import slab
            ex = getattr(self, "_slab_ex", None)           # one exchange object per (model, group): its gather / receive buffers are persistent
            if ex is None or ex.group is not self.view_group:
                ex = self._slab_ex = slab.DistExchange(self.view_group)
            if ex.G > 1 and slab.can_shard(ht // factor, ex.G):
                return slab.sharded_forward(self, images, poses, intrinsics, scale, ex)
        poses, intrinsics, s = scaled_cameras(poses, intrinsics, scale, factor)
        if ht % factor or wd % factor:
            raise RuntimeError(f"RAFT.forward: image size {wd}x{ht} must be a multiple of {factor} (the cost volume lives at 1/{factor} "
                               "resolution; the reference crops / rescales to such sizes, utils/data_utils.py:58-78)")
        images = images.float()                           # (normalised to [-1,1] inside the encoders' stem kernel)
        h, w = ht // factor, wd // factor

        # ---- view sharding: this rank encodes and builds the partial view-sum over its own source views only
        V = num - 1
        views = cdist.local_views(V, self.view_group)
        # (uploaded BEFORE the encoders are enqueued: a pageable H2D copy is stream-ordered and would block the host
        # until everything enqueued so far has finished)
        Pij = pij_matrices(poses[0], intrinsics[0], [0] * len(views), views).to(dev) if views else None
        disp = torch.zeros(h * w, device=dev, dtype=torch.float32)
        if self._split_path(dev, V):
            net_l, inp_l, split = self._encode_direct_split(images, V, h, w)
            f1, f2 = split[0], None                       # (cost_build takes the device from its first argument; the rows are never read)
        else:
            net_l, inp_l, f1, f2 = self.encode(images, views, raw=True)
            split = None
        del images
        return self._run_stages(net_l, inp_l, f1, f2, split, Pij, disp, views, V, h, w, do_report) * s

    def forward_cached(self, ref_image, f1s, store, slots, poses, intrinsics, scale):
        """A test-mode forward whose fnet features already exist (scan.ScanSession): ``ref_image`` [1,3,H,W] (or [3,H,W]) raw 0..255, the
        reference view, for ``cnet``; ``f1s`` [h*w,128] f16, the reference view's split-f16 operand planes (ops.feat_ref_rows of its
        block); ``store`` [M,(h+4)*(w+4),128] f16, bordered blocks as ``HipEncoder.features_split`` writes them; ``slots`` int32 [V] on
        the device: source view v is block slots[v].  ``poses`` [1,1+V,4,4], ``intrinsics`` [1,1+V,3,3], reference view first, as
        ``forward`` takes them.  Same stages, same bits and same result as ``forward`` on the stack of those images - without its
        1 + V fnet passes.  Needs ``supports_cached`` and a decided arithmetic form."""
        dev = ref_image.device
        if not self.supports_cached(dev):
            raise RuntimeError("RAFT.forward_cached: this model's forward does not take the direct-split path (see supports_cached)")
        if self.gru_precision == "auto" and self._auto_pending():
            raise RuntimeError("RAFT.forward_cached: gru_precision='auto' is still calibrating these weights; run ordinary forwards first")
        if scale is None:
            raise AssertionError("scale is required in test mode (reference: core/raft.py:107)")
        return self._with_policy(dev, lambda: self._forward_cached(ref_image, f1s, store, slots, poses, intrinsics, scale))

    def _forward_cached(self, ref_image, f1s, store, slots, poses, intrinsics, scale):
        self._validate_packs()
        dev = ref_image.device
        if ref_image.dim() == 3:
            ref_image = ref_image[None]
        ht, wd = ref_image.shape[-2:]
        poses, intrinsics, s = scaled_cameras(poses, intrinsics, scale, 4)
        if ht % 4 or wd % 4:
            raise RuntimeError(f"RAFT.forward_cached: image size {wd}x{ht} must be a multiple of 4")
        h, w = ht // 4, wd // 4
        V = int(slots.numel())
        if V < 1 or poses.shape[1] != 1 + V or intrinsics.shape[1] != 1 + V:
            raise RuntimeError("RAFT.forward_cached: poses and intrinsics must hold the reference view and one entry per slot")
        if store.dim() != 3 or tuple(store.shape[1:]) != ((h + 4) * (w + 4), 128) or f1s.numel() != h * w * 128:
            raise RuntimeError("RAFT.forward_cached: f1s / store do not fit the reference image's feature grid")
        views = list(range(1, V + 1))                     # (1-based: entry 0 of poses / intrinsics is the reference view)
        Pij = pij_matrices(poses[0], intrinsics[0], [0] * V, views).to(dev)
        disp = torch.zeros(h * w, device=dev, dtype=torch.float32)
        net_l, inp_l, _, _ = self._get_engines(dev)[2].context(ref_image.float(), raw=True)
        return self._run_stages(net_l, inp_l, f1s, None, (f1s, store, slots), Pij, disp, views, V, h, w) * s

    def _run_stages(self, net_l, inp_l, f1, f2, split, Pij, disp, views, V, h, w, do_report=False):
        """What follows the encoders in a single-GPU or view-sharded forward: the update block's loop objects, the hoisted convolutions,
        per stage the cost volume and the GRU iterations, the overflow policy's end-of-forward step -> disparity [1,1,h,w] (unscaled).
        What the encoders produced: ``net_l``, ``inp_l`` (context), ``f1`` / ``f2`` (fp32 reference / bordered source rows of this rank's
        ``views``) or ``split`` (the same as split-f16 operand planes with a view -> block map; None: formed here when a stage needs them).
        The geometry: ``Pij`` of ``views`` (this rank's, of V in all), the zeroed ``disp`` [h*w] that the stages update in place."""
        ub = self.update_block
        dev = disp.device
        if ub.conv_mode == "s16":
            try:
                for st_ in range(len(self.cascade)):
                    ub.loop(st_, dev)
            except RuntimeError as e:                     # weights that do not fit a shared split-f16 scale: wide-range kernels instead
                import warnings
                warnings.warn(f"cer-mvs_amd: {e}; this model runs with gru_precision='f16x3'")
                ub.conv_mode = "f16x3"
        net_l = ub.prepare_net(net_l, h, w)
        # split-f16 operand rows of the cost volume's MFMA products (csrc/cost_lines.hip): the same for every stage
        # (only when the epipolar-line-tile kernel will run for some stage: cer_feat_split_f16 is what raises overflow bit 1, and a
        # forward on the fp32 walk - cer_cost_build_algo(1), the remedy the overflow error names - must not be able to raise it)
        if split is None:
            lines = views and any(ops.on_line_tiles(self.dim_fmap, D_) for D_, _, _ in self.stages())
            split = (ops.feat_split(f1), ops.feat_split(f2)) if lines else None

        hoisted_all = ub.hoist_all(inp_l, h, w, len(self.cascade))
        ws = ub.workspace(h, w, dev)
        for stage, (D, incre, T) in enumerate(self.stages()):
            hoisted = hoisted_all[stage]
            single = self.view_group is None   # no cross-rank sum between the build and the pooling: fuse them
            # round 5: the folded volume keeps LEVEL 0 ONLY (rows of D instead of 1.75 D floats); the lookup kernel forms the pooled levels
            # on the fly, bit-identically (csrc/lookup.hip lk_elem) - less to write, to all-reduce (shard="views") and to read 32 times
            if views:
                vol, origin = ops.cost_build(f1, f2, Pij, disp, D, incre, stage == 0, h, w, ub.num_levels, fold=True,
                                             pyramid_scale=(1.0 / V) if (single and D <= 64) else None, split=split,
                                             src_hw=(h, w) if f2 is None else None, compact=True, two_term=self._cost_x2)
            else:                      # more ranks than views: contribute zeros
                _, _, rs = ops.row_layout(D, ub.num_levels, True)
                vol = torch.zeros(h * w, rs, device=dev)
                vol.level0_only = True
                origin = cdist.stage_origin(disp, D, incre, stage == 0)
            if not (single and views and D <= 64):
                cdist.reduce_volume(vol, self.view_group)
                ops.pyramid(vol, D, 1, scale=1.0 / V)
            if do_report and stage > 0:
                report()
            ub.run(T, vol, origin, net_l, disp, hoisted, stage, h, w, D, incre, ws)
        if self.overflow_policy == "lazy":
            ops.overflow_snapshot(dev)
        elif self.overflow_policy == "raise" and self.view_group is not None:
            # sharded by views: every rank reads its flag and the ranks agree (MAX) before anyone raises, so that no rank leaves the
            # collective sequence alone (the single-GPU form of "raise" / "fallback" is in forward())
            bits = cdist.max_int(int(ops.check_overflow(dev)), self.view_group, dev)
            if bits:
                self._raise_overflow(bits)
        return disp.view(1, 1, h, w)

    def _forward_literal(self, images, poses, intrinsics, scale, do_report):
        """Reference control flow call for call (CorrBlock per stage, per-view lookup, UpdateBlock.forward):
        used for non-"mean" aggregations and by the parity tests of the literal API."""
        dev = images.device
        factor = 8 if self.encoder_type == "LR" else 4
        poses, intrinsics, s = scaled_cameras(poses, intrinsics, scale, factor)
        batch, num, ch, ht, wd = images.shape
        images = images.float() * (2 / 255.0) - 1
        h, w = ht // factor, wd // factor
        disp = torch.zeros(batch, 1, h, w, device=dev)
        ctx = self.cnet(images[:, [0]]).float()
        net, inp = ctx.split([self.dim_net, self.dim_inp], dim=2)
        net, inp = torch.tanh(net), torch.relu(inp)
        ub = self.update_block
        V = num - 1
        sharded = self.view_group is not None and cdist.group_info(self.view_group)[0] > 1
        if sharded:
            # view sharding of the literal path (fallback for max / std aggregation): this rank encodes and
            # correlates ITS views; the looked-up [33, h, w] features are aggregated across ranks every GRU step
            views = cdist.local_views(V, self.view_group)
            sel = [0] + views
            images, poses, intrinsics = images[:, sel], poses[:, sel], intrinsics[:, sel]
        nloc = images.shape[1] - 1
        ii = torch.zeros(nloc, dtype=torch.long)
        jj = torch.arange(1, nloc + 1)
        fmaps = self.fnet(images).float()
        for stage, (D, incre, T) in enumerate(self.stages()):
            corr_fn = None
            if nloc:
                corr_fn = CorrBlock(fmaps, poses, intrinsics, ii, jj, nIncre=D, incre=incre, disps_input=disp.detach(),
                                    shift=(stage == 0), num_levels=ub.num_levels, radius=ub.radius, test_mode=True, do_report=do_report)
            for _ in range(T):
                if sharded:
                    K = ub.num_levels * (2 * ub.radius + 1)
                    frames = corr_fn(disp[:, ii.to(dev)])[0] if nloc else torch.zeros(0, K, h, w, device=dev)
                    net, delta = ub(net, inp, disp, None, stage, parts=cdist.aggregate_views(frames, V, ub.aggregation, self.view_group))
                else:
                    corr_frames = corr_fn(disp[:, ii.to(dev)])
                    net, delta = ub(net, inp, disp, corr_frames, stage)
                disp = disp + delta.float()
        assert s is not None
        return disp * s
