"""UpdateBlock / ConvGRU (reference: core/update.py:9-25, 29-120) on the HIP conv kernels.

Same constructor arguments, parameter names (state_dict keys) and ``forward(net, inp, disp,
corr_frames, stage) -> (net, delta)`` as the reference.  Internally activations are channels-last
[h*w, C]; one iteration of the update block is 6 kernel launches:

  lookup+mean+1x1+ReLU -> 3x3 64->64 ReLU -> {z,r} 3x3 (sigmoid, r*net) -> q 3x3 (tanh, GRU blend)
  -> delta 3x3 64->256 ReLU -> delta 3x3 256->1 (+ disp update)

Two exact algebraic reductions are used on the fast path (``step``): the GRU's `inp` slice of
convz/convr/convq is constant over iterations and stages, so its contribution is convolved once
per forward and fed to the MFMA accumulators as their initial value (``hoist``); and the 49-channel
disparity encoder is generated inside the conv kernel instead of being materialised."""
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import _lib as L
from . import ops


USE_PLANS = True         # replay recorded launches for GRU iterations 2..T (False: every iteration through the checked wrappers)
ALIAS_RN_C1 = True       # r*h shares c1's buffer (see _S16Loop.workspace; False: two independent buffers)


class ConvGRU(nn.Module):
    """Parameter container + literal forward (reference: core/update.py:9-25)."""

    def __init__(self, kernel_z=3, kernel_r=3, kernel_q=3, h_planes=None, i_planes=None):
        super().__init__()
        if (kernel_z, kernel_r, kernel_q) != (3, 3, 3):
            raise NotImplementedError("ConvGRU: only the reference's default 3x3 kernels are built")
        self.do_checkpoint = False
        self.h_planes, self.i_planes = h_planes, i_planes
        self.convz = nn.Conv2d(h_planes + i_planes, h_planes, 3, padding=1)
        self.convr = nn.Conv2d(h_planes + i_planes, h_planes, 3, padding=1)
        self.convq = nn.Conv2d(h_planes + i_planes, h_planes, 3, padding=1)
        self._packed = None

    def _apply(self, fn, *a, **k):
        self._packed = None
        return super()._apply(fn, *a, **k)

    def forward(self, net, *inputs):
        """net [1,Ch,h,w], inputs: NCHW tensors concatenated along channels (any split)."""
        x = torch.cat(inputs, dim=1)
        _, ch, h, w = net.shape
        cx = x.shape[1]
        cpad = (cx + 31) // 32 * 32
        dev = net.device
        if self._packed is None or self._packed[0] != (cx, dev):
            wzr = torch.cat([self.convz.weight, self.convr.weight], 0)
            bzr = torch.cat([self.convz.bias, self.convr.bias], 0)
            srcs = [(ch, 0), (cx, 0)]
            pzr, pq = ops.PackedConv3x3(wzr, bzr, srcs, dev), ops.PackedConv3x3(self.convq.weight, self.convq.bias, srcs, dev)
            pzr.sources = pq.sources = [(ch, 0), (cpad, 0)]      # (packed for cx input channels, run on a zero-padded copy: row stride cpad)
            self._packed = ((cx, dev), pzr, pq)
        _, pzr, pq = self._packed
        net_l = ops.nchw_to_nhwc(net[0].float().contiguous())
        xp = torch.zeros(h * w, cpad, device=dev, dtype=torch.float32)
        xp[:, :cx] = ops.nchw_to_nhwc(x[0].float().contiguous())
        z, rn = ops.conv3x3(pzr, [net_l, xp], h, w, L.EPI_GATES, aux=net_l)
        new = ops.conv3x3(pq, [rn, xp], h, w, L.EPI_GRU, aux=net_l, aux2=z)
        return ops.nhwc_to_nchw(new).view(1, ch, h, w)


def _stage_weights(ub, stage, device):
    """The weights of ``stage``; GRU input channels net | inp | disp49 | corr (core/update.py:18-19,112): ``inp`` is hoisted, ``rest`` looped."""
    ce, gru, de = (getattr(ub, n) for n in ub._names(stage))
    f32 = lambda t: t.detach().to(device, torch.float32).contiguous()
    wzr = torch.cat([gru.convz.weight, gru.convr.weight], 0).detach()
    return SimpleNamespace(w0t=f32(ce[0].weight[:, :, 0, 0].t()), b0=f32(ce[0].bias), corr2=ce[2], delta1=de[0], delta2=de[2],
                           d2b=float(de[2].bias.detach().float().cpu()[0]), wzr=wzr, bzr=torch.cat([gru.convz.bias, gru.convr.bias], 0).detach(),
                           wq=gru.convq.weight.detach(), bq=gru.convq.bias.detach(), inp=slice(64, 128),
                           rest=list(range(0, 64)) + list(range(128, wzr.shape[1])))


class _S16Loop:
    """gru_precision "s16" / "s16f8" / "s16f6": split-f16 MFMA kernels with one accumulator (csrc/conv_s16.hip).  Every loop tensor lives in HBM
    in the split16 layout with a per-class power-of-two scale (hidden state and r*h: |x| <= 1; ReLU outputs; generated disparity features), over
    whole m-tiles (ops.s16_pixels).  PackedConvS16 raises when the weights of one conv do not fit a shared scale (cer_conv3x3_s16_scale): RAFT
    sees that error when it builds the loops and switches ``conv_mode`` to "f16x3" (with a warning)."""

    # the disparity update of iteration i (the 18-tap gather of the fused delta head's tap planes, ``ops.delta_sum``) rides on the lookup launch of
    # iteration i + 1 (csrc/lookup.hip, round 5): one launch less per iteration; the last iteration of a stage ends with the stand-alone kernel.
    # Off where something reads ``disp`` between two iterations (the row-slab exchange: ``run(after=...)``).
    FUSE_DELTA = True

    def __init__(self, ub, stage, device, corr_fp8):
        g = _stage_weights(ub, stage, device)
        U, R, Dp = L.S16_UNIT, L.S16_RELU, L.S16_DISP
        loop_src = [(64, 2, U), (49, 1, Dp), (64, 2, R)]           # (net | disp49 | corr; widths fixed by UpdateBlock)
        pack = lambda wt, b, srcs: ops.PackedConvS16(wt, b, srcs, device, corr_fp8=corr_fp8)
        self.num_levels, self.radius, self.w0t, self.b0, self.d2b, self.ws_cache = ub.num_levels, ub.radius, g.w0t, g.b0, g.d2b, ub._ws_cache
        self.corr2 = pack(g.corr2.weight, g.corr2.bias, [(64, 2, R)])
        self.zr, self.q = pack(g.wzr[:, g.rest], None, loop_src), pack(g.wq[:, g.rest], None, loop_src)
        self.zr_inp, self.q_inp = pack(g.wzr[:, g.inp], g.bzr, [(64, 2, R)]), pack(g.wq[:, g.inp], g.bq, [(64, 2, R)])
        self.d1 = pack(g.delta1.weight, g.delta1.bias, [(64, 2, U)])
        self.d2proj = ops.delta_proj_pack_s16(g.delta2.weight, device)

    def hoist(self, inp_l, h, w):         # (the results are in the acc32 layout: they seed the accumulators of the loop's convs)
        inp_s = ops.to_frag16(inp_l, h, w, L.S16_RELU)
        ops.scan_overflow(inp_s)              # (a ReLU-class tensor: saturation must not be silent, see ``finish``)
        return (ops.conv3x3_s16(self.zr_inp, [inp_s], h, w, L.EPI_LINEAR), ops.conv3x3_s16(self.q_inp, [inp_s], h, w, L.EPI_LINEAR))

    def prepare_net(self, net_l, h, w):
        return ops.to_frag16(net_l, h, w, L.S16_UNIT)

    def workspace(self, h, w, device):
        # persistent per (size, device), on the UpdateBlock: allocated (and zero-filled) once - 4 x 30 MB of memsets per forward otherwise;
        # every data pixel is overwritten by the first iteration of a forward, the padding slots are never consumed (see below)
        cache, key = self.ws_cache, (h, w, str(device))
        if key not in cache:
            while len(cache) >= 8:            # (row slabs of different heights share a process in the simulated-rank tests)
                cache.pop(next(iter(cache)))
            z = lambda c: torch.zeros(ops.s16_pixels(h, w), c, device=device, dtype=torch.float32)
            cache[key] = {"c1": z(64), "c2": z(64), "z": z(64), "T": torch.empty(2, 9, h * w, device=device, dtype=torch.float32)}
            # r*h is written by the z|r launch, after the only reader of c1 (the corr2 launch) has run, and read by the q launch, before the
            # next lookup writes c1 again: with ALIAS_RN_C1 the two tensors ARE ONE 30 MB buffer (ws["rn"] is ws["c1"]; round 5: the iteration's
            # working set - 283 MB at 296 x 400 - sits just above the 256 MB Infinity Cache).  Legal because nothing reads c1 behind the z|r
            # launch of an iteration.  (The padding slots of these tensors need NOT stay zero: the epilogues store whole m-tiles, and every
            # consumer masks pixels outside the image while it stages; tests/test_conv_s16_gpu.py::test_rn_may_share_c1s_buffer runs a forward
            # on a garbage-filled workspace.)  Tools that want two independent buffers set update.ALIAS_RN_C1 = False.
            cache[key]["rn"] = cache[key]["c1"] if ALIAS_RN_C1 else z(64)
        return cache[key]

    def step(self, vol, origin, net_l, disp, hoisted, h, w, D, incre, ws, delta="now"):
        U, R = L.S16_UNIT, L.S16_RELU
        hzr, hq = hoisted
        ops.lookup_encode(vol, origin, disp, self.w0t, self.b0, D, incre, self.num_levels, self.radius, out=ws["c1"], out_split=2, log2s=R,
                          img_w=w, delta=(ws["T"], self.d2b) if delta == "apply+defer" else None)
        ops.conv3x3_s16(self.corr2, [ws["c1"]], h, w, L.EPI_RELU, out=ws["c2"], out_split=True, log2s_out=R)
        ops.conv3x3_s16(self.zr, [net_l, disp, ws["c2"]], h, w, L.EPI_GATES, out=ws["z"], out2=ws["rn"], aux=net_l, init=hzr,
                        log2s_out=U, log2s_aux=U)
        ops.conv3x3_s16(self.q, [ws["rn"], disp, ws["c2"]], h, w, L.EPI_GRU, out=net_l, aux=net_l, aux2=ws["z"], init=hq,
                        log2s_out=U, log2s_aux=U)
        ops.conv3x3_s16(self.d1, [net_l], h, w, L.EPI_DELTA, out=ws["T"], aux=self.d2proj)
        if delta == "now":
            ops.delta_sum(ws["T"], self.d2b, disp, h, w, disp_out=disp, want_delta=False)

    def finish(self, ws):
        """After a stage's last iteration, on both forwards: a hook, intentionally empty - every launch of the loop checks what it clamps
        itself (c1 and c2: bit 4, the delta head's hidden map: bit 2, the disparity: bit 8), so nothing is left to scan."""

    def rows(self, h, w):       # row mover of the m-tile-major hidden state for the slab exchange
        return lambda t, flat, y0, nr, to_t: ops.s16_rows(t, flat, h, w, y0, nr, to_t)


class _WideLoop:
    """gru_precision "f16x3" (round-1 split-f16 kernels, two accumulators) or "fp32" on the general kernels (ops.conv3x3).  f16x3: the loop's
    activations (hidden state, corr features, r*h) live in HBM in the "split32" layout - hi|lo f16 pairs in the fp32 slots (cer_mvs.h) - written by
    the producers' epilogues, so that every conv stages its tensor sources with plain 16-byte copies instead of re-splitting them (staging was ~10 %
    of the conv time, VALU-bound): the hidden state is carried at 2^-22 relative resolution, the resolution the f16x3 products see anyway.
    ``literal``: the packs of ``UpdateBlock.forward`` (GRU convs over all inputs)."""

    FUSE_DELTA = False

    def __init__(self, ub, stage, device, mode, literal=False):
        g = _stage_weights(ub, stage, device)
        pack = lambda wt, b, srcs: ops.PackedConv3x3(wt, b, srcs, device)
        self.mode, self.num_levels, self.radius, self.w0t, self.b0, self.d2b = mode, ub.num_levels, ub.radius, g.w0t, g.b0, g.d2b
        self.corr2 = pack(g.corr2.weight, g.corr2.bias, [(64, 0)])
        if literal:
            full_src = [(64, 0), (64, 0), (49, 1), (64, 0)]
            self.zr, self.q = pack(g.wzr, g.bzr, full_src), pack(g.wq, g.bq, full_src)
        else:
            loop_src = [(64, 0), (49, 1), (64, 0)]
            self.zr, self.q = pack(g.wzr[:, g.rest], None, loop_src), pack(g.wq[:, g.rest], None, loop_src)
            self.zr_inp, self.q_inp = pack(g.wzr[:, g.inp], g.bzr, [(64, 0)]), pack(g.wq[:, g.inp], g.bq, [(64, 0)])
        self.d1 = pack(g.delta1.weight, g.delta1.bias, [(64, 0)])
        if mode == "f16x3":
            self.d2proj = ops.delta_proj_pack(g.delta2.weight, device)
        else:
            self.d2w = g.delta2.weight.detach()[0].permute(1, 2, 0).reshape(9, -1).to(device, torch.float32).contiguous()    # [tap, C]

    def hoist(self, inp_l, h, w):
        return (ops.conv3x3(self.zr_inp, [inp_l], h, w, L.EPI_LINEAR, mode=self.mode),
                ops.conv3x3(self.q_inp, [inp_l], h, w, L.EPI_LINEAR, mode=self.mode))

    def prepare_net(self, net_l, h, w):
        return ops.split32(net_l) if self.mode == "f16x3" else net_l

    def workspace(self, h, w, device):
        e = lambda *shape: torch.empty(*shape, device=device, dtype=torch.float32)
        ws = {k: e(h * w, 64) for k in ("c1", "c2", "z", "rn")}
        ws.update({"T": e(2, 9, h * w)} if self.mode == "f16x3" else {"hid": e(h * w, 256)})
        return ws

    def step(self, vol, origin, net_l, disp, hoisted, h, w, D, incre, ws, delta="now"):
        hzr, hq = hoisted
        # corr2, z|r and q run on the f16x3 kernel in both modes: what the "fp32" form has always launched (its hoisted term and its delta
        # head are the exact fp32 ones).  f16x3: the loop's tensors are in the split32 layout (kind 3 sources, split results)
        split = self.mode == "f16x3"
        one, three = ([3], [3, 1, 3]) if split else (None, None)      # source kinds of the one- and the three-source convs
        ops.lookup_encode(vol, origin, disp, self.w0t, self.b0, D, incre, self.num_levels, self.radius, out=ws["c1"], out_split=split)
        ops.conv3x3(self.corr2, [ws["c1"]], h, w, L.EPI_RELU, mode="f16x3", out=ws["c2"], kinds=one, out_split=split)
        ops.conv3x3(self.zr, [net_l, disp, ws["c2"]], h, w, L.EPI_GATES, mode="f16x3", out=ws["z"], out2=ws["rn"], aux=net_l, init=hzr,
                    kinds=three, out_split=split, aux_split=split)
        ops.conv3x3(self.q, [ws["rn"], disp, ws["c2"]], h, w, L.EPI_GRU, mode="f16x3", out=net_l, aux=net_l, aux2=ws["z"], init=hq,
                    kinds=three, out_split=split, aux_split=split)
        self.delta_head(net_l, disp, h, w, buf=ws["T" if split else "hid"], kinds=one, disp_out=disp, want_delta=False)

    def delta_head(self, net_l, disp, h, w, buf=None, kinds=None, disp_out=None, want_delta=True):
        """delta 3x3 64 -> 256 ReLU, 3x3 256 -> 1, disparity update -> (disp_out, delta or None).  f16x3: the projection rides in the first
        conv's epilogue (EPI_DELTA: tap planes, summed by ``delta_sum``); fp32: the hidden map, then ``delta_tail``.  ``buf``: where the tap
        planes / the hidden map go (the loop's workspace; None: a new tensor); ``kinds``: [3] when ``net_l`` is in the split32 layout."""
        if self.mode == "f16x3":
            T = ops.conv3x3(self.d1, [net_l], h, w, L.EPI_DELTA, mode="f16x3", out=buf, aux=self.d2proj, kinds=kinds)
            return ops.delta_sum(T, self.d2b, disp, h, w, disp_out=disp_out, want_delta=want_delta)
        hid = ops.conv3x3(self.d1, [net_l], h, w, L.EPI_RELU, mode="fp32", out=buf)
        return ops.delta_tail(hid, self.d2w, self.d2b, disp, h, w, disp_out=disp_out, want_delta=want_delta)

    def finish(self, ws):       # (no clamping layouts)
        pass

    def rows(self, h, w):       # (row-major hidden state: the slab exchange copies plain rows)
        return None


class UpdateBlock(nn.Module):
    def __init__(self, kernel_corr=3, dim0_corr=64, dim1_corr=64, dim_net=None, dim_inp=None, dim0_delta=256,
                 kernel0_delta=3, kernel1_delta=3, num_levels=3, radius=5, size_disp_enc=7, kernel0_vis=3, kernel1_vis=3,
                 share_corr=True, share_gru=True, share_delta=False, aggregation=("mean",), cascade=None):
        super().__init__()
        if (kernel_corr, kernel0_delta, kernel1_delta, size_disp_enc) != (3, 3, 3, 7):
            raise NotImplementedError("UpdateBlock: only the reference's default kernel sizes are built")
        if (dim0_corr, dim1_corr, dim_net, dim_inp, dim0_delta) != (64, 64, 64, 64, 256):
            raise NotImplementedError("UpdateBlock: only the reference's default widths (64/64/64/64/256) are built")
        self.num_levels, self.radius, self.size_disp_enc = num_levels, radius, size_disp_enc
        self.share_corr, self.share_gru, self.share_delta = share_corr, share_gru, share_delta
        self.aggregation = list(aggregation)
        self.cascade = cascade
        self.dim_net, self.dim_inp = dim_net, dim_inp
        cor_planes = len(self.aggregation) * num_levels * (2 * radius + 1)
        n_cascade = len(cascade)
        for i in (range(n_cascade) if not share_corr else [""]):
            setattr(self, f"corr_encoder{i}", nn.Sequential(
                nn.Conv2d(cor_planes, dim0_corr, 1, padding=0), nn.ReLU(inplace=True),
                nn.Conv2d(dim0_corr, dim1_corr, 3, padding=1), nn.ReLU(inplace=True)))
        for i in (range(n_cascade) if not share_delta else [""]):
            setattr(self, f"delta{i}", nn.Sequential(
                nn.Conv2d(dim_net, dim0_delta, 3, padding=1), nn.ReLU(inplace=True), nn.Conv2d(dim0_delta, 1, 3, padding=1)))
        i_planes = dim_inp + dim1_corr + size_disp_enc ** 2
        for i in (range(n_cascade) if not share_gru else [""]):
            setattr(self, f"gru{i}", ConvGRU(h_planes=dim_net, i_planes=i_planes))
        # arithmetic of the 3x3 convolutions: "s16" (split-f16 MFMA, one accumulator, barrier-light kernels of conv_s16.hip: the
        # fast path), "f16x3" (round-1 split-f16 kernels, two accumulators) or "fp32" (exact fp32 MFMA)
        self.conv_mode = "s16"
        self._loops = {}        # ``loop`` objects: caches of the parameters
        self._ws_cache = {}     # s16 workspaces per (h, w, device): independent of the weights
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.refresh_weights())

    # s16 path: the two correction terms of the split-f16 product (2^-11 of the main term) of every tensor source on the block-scaled
    # fp8 matrix instruction (twice the f16 rate): gru_precision="s16f8".  End to end 4e-6 instead of 2e-7 relative L1 from fp32.
    corr_fp8 = False

    def refresh_weights(self):
        """Drop packed weights (call after mutating parameters)."""
        self._loops = {}
        for m in self.modules():
            if isinstance(m, ConvGRU):
                m._packed = None

    def _apply(self, fn, *a, **k):
        self._loops = {}
        return super()._apply(fn, *a, **k)

    def _names(self, stage):
        return (f"corr_encoder{stage if not self.share_corr else ''}", f"gru{stage if not self.share_gru else ''}",
                f"delta{stage if not self.share_delta else ''}")

    def loop(self, stage, device, literal=False):
        """The GRU loop of ``stage`` on ``device`` in the current arithmetic form (``conv_mode``, ``corr_fp8``), with the packed weights
        its launches read: built once, cached.  ``literal``: the packs of ``forward``, which runs on the general round-1 kernels."""
        f8 = 6 if self.corr_fp8 == 6 else bool(self.corr_fp8)      # (False: three f16 terms, True: fp8 corrections, 6: FP6 corrections)
        mode = "f16x3" if literal and self.conv_mode == "s16" else self.conv_mode
        key = (stage, str(device), mode, f8, literal)
        if key not in self._loops:
            self._loops[key] = _S16Loop(self, stage, device, f8) if mode == "s16" else _WideLoop(self, stage, device, mode, literal)
        return self._loops[key]

    def packed(self, stage, device):
        """Packed weights of ``stage``'s loop on ``device`` by name (w0t, b0, d2b, the convs' packs)."""
        return vars(self.loop(stage, device))

    # ------------------------------------------------------------------ fast path (channels-last)
    def hoist_all(self, inp_l, h, w, n_stages):
        """Contribution of the constant `inp` slice (+ biases) to the z|r and q pre-activations, per cascade stage: one result shared by all
        stages when the GRU weights are shared (the reference's default, core/update.py:47), else one per stage (gru{stage}'s own weights)."""
        if self.share_gru:
            return [self.loop(0, inp_l.device).hoist(inp_l, h, w)] * n_stages
        return [self.loop(s, inp_l.device).hoist(inp_l, h, w) for s in range(n_stages)]

    def prepare_net(self, net_l, h, w):
        """Hidden state [h*w,64] fp32 -> the layout ``step`` keeps it in (frag16 on the s16 path, split32 on the f16x3 path)."""
        return self.loop(0, net_l.device).prepare_net(net_l, h, w)

    def step(self, vol, origin, net_l, disp, hoisted, stage, h, w, D, incre, ws, delta="now"):
        """One GRU iteration on the folded volume; updates ``net_l`` [P,64] (see ``prepare_net``) and ``disp`` [P] in place.  ``ws``: ``workspace``.
        ``delta`` (s16 path): "now" - the disparity update is a launch of its own at the end of the step; "defer" - it is left pending in ``ws["T"]``
        for the next step's lookup; "apply+defer" - this step's lookup first applies the pending update of the previous step, and leaves its own."""
        self.loop(stage, net_l.device).step(vol, origin, net_l, disp, hoisted, h, w, D, incre, ws, delta)

    def run(self, iters, vol, origin, net_l, disp, hoisted, stage, h, w, D, incre, ws, after=None):
        """``iters`` GRU iterations on fixed buffers: the first executes through the checked wrappers while its raw launches are recorded
        (``_lib.LaunchPlan``), the rest replay them.  ``after(i)``: called after every iteration (the slab exchange of the sharded forward)."""
        plan = None
        loop = self.loop(stage, net_l.device)   # weight packing (host work) must not end up in the recorded plan
        args = (vol, origin, net_l, disp, hoisted, h, w, D, incre, ws)
        fuse = loop.FUSE_DELTA and after is None and iters >= 2
        for i in range(iters):
            mode = ("defer" if i == 0 else "apply+defer") if fuse else "now"
            if not USE_PLANS or mode == "defer":  # (fused: nothing pending yet - through the checked wrappers, its update left pending)
                loop.step(*args, delta=mode)
            elif plan is None:
                plan = L.LaunchPlan(keep=(vol, origin, net_l, disp, hoisted, ws))
                with L.recording(plan):
                    loop.step(*args, delta=mode)
            else:
                plan.replay()
            if after is not None:
                after(i)
        if fuse:                                # the last iteration's update
            ops.delta_sum(ws["T"], loop.d2b, disp, h, w, disp_out=disp, want_delta=False)
        if iters > 0:
            loop.finish(ws)

    def workspace(self, h, w, device):
        """Scratch tensors of the loop for an h x w image (s16 path: m-tile-major layouts over whole m-tiles, ops.s16_pixels)."""
        return self.loop(0, device).workspace(h, w, device)

    # ------------------------------------------------------------------ literal API
    def disp_encoder(self, disp):
        """[B,1,h,w] -> [B,49,h,w] (reference: core/update.py:80-85); not used by the HIP path, which
        generates these channels inside the conv kernel."""
        batch, _, ht, wd = disp.shape
        k = self.size_disp_enc
        u = torch.nn.functional.unfold(disp, [k, k], padding=k // 2).view(batch, k * k, ht, wd)
        return u - disp.view(batch, 1, ht, wd)

    def forward(self, net, inp, disp, corr_frames, stage, parts=None):
        """net, inp [B,num,64,h,w]; disp [B,1,h,w]; corr_frames [B,V,33,h,w] -> (net [B,num,64,h,w], delta [B,num,h,w]).
        ``parts`` (extension): the view aggregates [33,h,w] in the order mean, max, std, already reduced over all views - the
        view-sharded literal forward passes them (dist.aggregate_views) instead of ``corr_frames``."""
        if not net.is_cuda:
            raise RuntimeError("net must be a CUDA tensor")
        batch, num, ch, ht, wd = net.shape
        if batch * num != 1:
            raise RuntimeError("UpdateBlock.forward: batch*num must be 1")
        P = ht * wd
        dev = net.device
        p = self.loop(stage, dev, literal=True)
        net_l = ops.nchw_to_nhwc(net.reshape(ch, P).float().contiguous())
        inp_l = ops.nchw_to_nhwc(inp.reshape(-1, P).float().contiguous())
        disp_l = disp.reshape(P).float().contiguous()
        if parts is None and self.aggregation == ["mean"]:
            feats = corr_frames[0].float()
            c1 = ops.corr_encode(feats.reshape(feats.shape[0], -1, P).contiguous(), p.w0t, p.b0)
        else:
            if parts is None:
                feats = corr_frames[0].float()
                parts = [torch.mean(feats, dim=0)] if "mean" in self.aggregation else []
                parts += [torch.max(feats, dim=0).values] if "max" in self.aggregation else []
                parts += [torch.std(feats, dim=0)] if "std" in self.aggregation else []
            # stack(dim=2).view(...) in the reference interleaves [part][channel]: channel-major then part
            agg = torch.stack([t.float() for t in parts], dim=1).reshape(1, -1, P).contiguous()
            c1 = ops.corr_encode(agg, p.w0t, p.b0)
        c2 = ops.conv3x3(p.corr2, [c1], ht, wd, L.EPI_RELU, mode=p.mode)
        z, rn = ops.conv3x3(p.zr, [net_l, inp_l, disp_l, c2], ht, wd, L.EPI_GATES, mode=p.mode, aux=net_l)
        new = ops.conv3x3(p.q, [rn, inp_l, disp_l, c2], ht, wd, L.EPI_GRU, mode=p.mode, aux=net_l, aux2=z)
        _, delta = p.delta_head(new, disp_l, ht, wd)
        net_out = ops.nhwc_to_nchw(new).view(batch, num, ch, ht, wd)
        return net_out, delta.view(batch, num, ht, wd)
