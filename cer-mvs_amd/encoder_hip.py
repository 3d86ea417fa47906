"""BasicEncoder forward on the HIP encoder engine (csrc/enc_conv.hip) - reference: core/extractor.py:143-155 (type "HR").

Same arithmetic as ``BasicEncoder.forward`` (conv7x7s2 -> norm -> relu -> 2 residual blocks @32 -> 2 residual blocks @64
(first stride 2 with a 1x1 downsample) -> conv1x1), re-scheduled so that no normalised / activated tensor is ever written:
each convolution stores its RAW output plus per-block statistics partials, and the consumer applies
``relu((x - mean) * rstd)`` while it stages its input tile.  Activations are channels-last fp32; convolutions run on
the split-f16 MFMA path (fp32-equivalent).  Only "instance" and "none" norms (the two the reference uses) are built."""
import ctypes

import torch

from . import _lib as L
from .ops import pack_host

# "pc" (round 4, default): producer / consumer convolutions with the residual merges formed on the fly (csrc/enc_pc.hip);
# "tiled": the round-2/3 kernels (csrc/enc_conv.hip: every wave runs every phase; separate enc_merge passes) - the cross-reference of "pc"
# (tests/test_encoder_parity_gpu.py sets it)
ENGINE = "pc"


class _In:
    """A block input that is not (necessarily) materialised: x = relu_s( relu_a(n(A)) + relu_b(n(B)) ), B optional."""
    __slots__ = ("A", "sA", "rA", "B", "sB", "rB", "C")

    def __init__(self, A, sA, rA, C, B=None, sB=None, rB=False):
        self.A, self.sA, self.rA, self.B, self.sB, self.rB, self.C = A, sA, rA, B, sB, rB, C

    def images(self, n0, n1):
        sl = lambda t: None if t is None else t[n0:n1]
        ss = lambda t: None if t is None else t[n0 * self.C:n1 * self.C]
        return _In(sl(self.A), ss(self.sA), self.rA, self.C, sl(self.B), ss(self.sB), self.rB)

    def flags(self):
        """The producer flags of cer_enc_pc_conv and cer_enc_merge_f32: 1 = relu on A, 2 = relu on B, 4 = there is a B (sum, then relu)."""
        return (1 if self.rA else 0) | ((2 if self.rB else 0) | 4 if self.B is not None else 0)


class _Conv:
    def __init__(self, conv, device):
        lib = L.load()
        w = conv.weight.detach().to("cpu", torch.float32).contiguous()
        self.cout, self.cin, k, _ = w.shape
        self.taps = k * k
        self.stride = conv.stride[0]
        wp, shape = ctypes.c_void_p(w.data_ptr()), (self.cout, self.cin, self.taps)
        size = lib.cer_enc_conv_packed_size(*shape)
        what = f"encoder conv pack: unsupported {tuple(w.shape)}"
        self.packed = pack_host(size, torch.float16, lambda p: lib.cer_enc_conv_pack(wp, p, *shape), what, device)
        # the same weights in the FP6-correction form (csrc/enc_pc.hip, round 6): same size and plane order, the lo planes as e2m3 K blocks
        self.packed_f6 = pack_host(size, torch.float16, lambda p: lib.cer_enc_conv_pack_f6(wp, p, *shape), what, device)
        self.bias = conv.bias.detach().to(device, torch.float32).contiguous()


class HipEncoder:
    """Runs one BasicEncoder ("HR", norm "instance" or "none") on the engine.  Weights are packed at construction."""

    def __init__(self, enc, device):
        if enc.type != "HR" or enc.norm_fn not in ("instance", "none"):
            raise NotImplementedError("HipEncoder: only type 'HR' with norm 'instance' or 'none'")
        self.inorm = enc.norm_fn == "instance"
        self.device = device
        # arithmetic of the producer / consumer convolutions: False = three f16 MFMA terms per product (fp32-class), True = the correction
        # terms on the FP6 form of the block-scaled matrix instruction (half the matrix cycles; RAFT sets it per forward: enc_precision)
        self.f6 = False
        # the 7x7 stem runs on the matrix cores (csrc/enc_stem.hip: cer_enc_stem_s16)
        self.stem_b = enc.conv1.bias.detach().to(device, torch.float32).contiguous()
        lib = L.load()
        wc = enc.conv1.weight.detach().to("cpu", torch.float32).contiguous()
        k = ctypes.c_int(0)
        self.stem_packed = pack_host(lib.cer_enc_stem_s16_packed_size(), torch.float16,
                                     lambda p: lib.cer_enc_stem_s16_pack(ctypes.c_void_p(wc.data_ptr()), p, ctypes.byref(k)),
                                     "encoder stem pack: unsupported", device)
        self.stem_log2s = int(k.value)
        self.blocks = []
        for layer in (enc.layer1, enc.layer2):
            for blk in layer:
                down = _Conv(blk.downsample[0], device) if blk.downsample is not None else None
                self.blocks.append((_Conv(blk.conv1, device), _Conv(blk.conv2, device), down))
        self.head = _Conv(enc.conv2, device)
        # what the producer / consumer engine serves (csrc/enc_pc.hip: cer_enc_pc_supported): the trunk's convolutions are fixed by the
        # encoder type, but the head is Conv2d(64, output_dim, 1) - `dim_fmap` / `dim_net + dim_inp` are constructor arguments of the
        # reference's RAFT (core/raft.py:14-30).  Anything it refuses runs on the tiled engine (csrc/enc_conv.hip: any Cout % 64 == 0).
        sup = lambda c, epi: bool(lib.cer_enc_pc_supported(c.cin, c.cout, c.taps, c.stride, epi))
        self.pc_trunk = all(sup(c, 0) for blk in self.blocks for c in blk if c is not None)
        self.pc_head = {epi: sup(self.head, epi) for epi in (1, 2, 3)}       # FMAP, CTX (tanh | relu halves), FSPLIT

    def _on_pc(self, epi=0):
        """The launch with epilogue ``epi`` (0: a trunk convolution, else a head) runs on the producer / consumer engine."""
        return ENGINE == "pc" and self.pc_trunk and (epi == 0 or self.pc_head[epi])

    # ---- kernel faces
    def _stats(self, part, N, C, pixels):
        """statistics partials [N, blocks, C, 2] of a launch (None: not asked for) -> (mean, rstd) [N*C, 2]"""
        if part is None:
            return None
        st = torch.empty(N * C, 2, device=self.device, dtype=torch.float32)
        L.check(L.load().cer_enc_stats_reduce_f32(L.dev_ptr(part, "part"), L.dev_ptr(st, "stats"), N, part.shape[1], C, pixels, 1e-5, L.cur_stream()),
                "enc_stats_reduce")
        return st

    def _launch(self, c, x, N, h, w, merged=False, epi=0, out=None, out2=None, border=0, scale=1.0, want_stats=True):
        """conv ``c`` of the (virtual) input ``x`` on the engine that serves it -> (raw out, stats, ho, wo, merged activation or None).
        The tiled engine reads one tensor: a two-tensor ``x`` goes through ``_materialise`` first.  ``epi`` 3 (the split feature head,
        producer / consumer engine only): ``out`` holds halves and the device's overflow flag (int32) takes ``out2``'s place."""
        lib = L.load()
        pc = self._on_pc(epi)
        if not pc and (x.B is not None or merged or epi == 3):
            raise RuntimeError("encoder: the tiled engine convolves one materialised tensor into fp32 outputs")
        pad, ks = (1, 3) if c.taps == 9 else (0, 1)
        ho, wo = (h + 2 * pad - ks) // c.stride + 1, (w + 2 * pad - ks) // c.stride + 1
        part = None
        if epi == 0:
            out = torch.empty(N, ho * wo, c.cout, device=self.device, dtype=torch.float32)
            if self.inorm and want_stats:
                nblk = lib.cer_enc_pc_tiles(ho, wo, c.cout, c.taps, c.stride) if pc else lib.cer_enc_conv_tiles(ho, wo, c.stride, c.taps, c.cout)
                part = torch.empty(N, nblk, c.cout, 2, device=self.device, dtype=torch.float32)
        t_out, t_out2 = (torch.float16, torch.int32) if epi == 3 else (torch.float32, torch.float32)
        tail = (L.dev_ptr(c.bias, "bias"), L.dev_ptr(out, "out", t_out), L.dev_ptr(out2, "out2", t_out2), L.dev_ptr(part, "part"),
                N, h, w, c.cin, c.cout, c.taps, c.stride, epi, border, float(scale), L.cur_stream())
        m = None
        if pc:
            if merged:
                m = torch.empty(N, h * w, c.cin, device=self.device, dtype=torch.float32)
            L.check(lib.cer_enc_pc_conv(L.dev_ptr(x.A, "srcA"), L.dev_ptr(x.sA, "statsA"), L.dev_ptr(x.B, "srcB"), L.dev_ptr(x.sB, "statsB"),
                                        x.flags() | (8 if self.f6 else 0), L.dev_ptr(m, "merged"),
                                        L.dev_ptr(c.packed_f6 if self.f6 else c.packed, "w", torch.float16), *tail), "enc_pc_conv")
        else:
            L.check(lib.cer_enc_conv_f16x3(L.dev_ptr(x.A, "src"), L.dev_ptr(x.sA, "tf"), int(x.rA), L.dev_ptr(c.packed, "w", torch.float16), *tail),
                    "enc_conv")
        return out, self._stats(part, N, c.cout, ho * wo), ho, wo, m

    def _merge(self, a, sa, b, sb, N, pixels, C, flags):
        out = torch.empty(N, pixels, C, device=self.device, dtype=torch.float32)
        L.check(L.load().cer_enc_merge_f32(L.dev_ptr(a, "a"), L.dev_ptr(sa, "sa"), L.dev_ptr(b, "b"), L.dev_ptr(sb, "sb"), L.dev_ptr(out, "out"),
                                           N, pixels, C, flags, L.cur_stream()), "enc_merge")
        return out

    def _materialise(self, x, N, pixels):
        """a two-tensor input as the plain tensor the tiled engine reads (one enc_merge pass)"""
        return _In(self._merge(x.A, x.sA, x.B, x.sB, N, pixels, x.C, x.flags()), None, False, x.C)

    def _stem(self, x, raw):
        lib = L.load()
        N, _, H, W = x.shape
        x = x.contiguous()
        ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        raw0 = torch.empty(N, ho * wo, 32, device=self.device, dtype=torch.float32)
        part = torch.empty(N, lib.cer_enc_stem_s16_tiles(ho, wo), 32, 2, device=self.device, dtype=torch.float32) if self.inorm else None
        L.check(lib.cer_enc_stem_s16(L.dev_ptr(x, "images"), L.dev_ptr(self.stem_packed, "w", torch.float16), L.dev_ptr(self.stem_b, "b"),
                                     L.dev_ptr(raw0, "out"), L.dev_ptr(part, "part"), N, H, W, int(bool(raw)), self.stem_log2s, L.cur_stream()),
                "enc_stem_s16")
        return raw0, self._stats(part, N, 32, ho * wo), ho, wo

    # ---- trunk: images -> the last residual block's output + geometry
    def _trunk_pc(self, x, raw=False):
        """x [N,3,H,W] float32, normalised to [-1,1] - or, with ``raw``, 0..255 pixel values that the stem kernel normalises while
        it loads them (x * 2/255 - 1, core/raft.py:40-41: no separate pass over the image stack) -> (the LAST residual block's output
        as a virtual input, h, w).  Producer / consumer engine: two tensors, merged by the consumer - 13.5 tensor passes over the
        half-resolution layer.  Tiled engine: every block's output is materialised, four merge passes - 16.25.  (The name is the
        producer / consumer walk's, which this is; the tiled engine's own walk was folded into it.)"""
        raw0, st0, h, w = self._stem(x, raw)
        N = x.shape[0]
        pc = self._on_pc()
        cur = _In(raw0, st0, True, 32)
        for c1, c2, down in self.blocks:
            keep = cur.B is not None and down is None                   # the skip branch needs the merged input as a tensor
            r1, s1, h1, w1, m = self._launch(c1, cur, N, h, w, merged=keep)
            r2, s2, _, _, _ = self._launch(c2, _In(r1, s1, True, c1.cout), N, h1, w1)
            if down is not None:
                rd, sd, _, _, _ = self._launch(down, cur, N, h, w)
                cur = _In(r2, s2, True, c2.cout, rd, sd, False)         # relu(norm3(down) + relu(norm(r2)))
            elif cur.B is None:
                cur = _In(r2, s2, True, c2.cout, cur.A, cur.sA, cur.rA)
            else:
                cur = _In(r2, s2, True, c2.cout, m, None, False)
            if not pc:
                cur = self._materialise(cur, N, h1 * w1)
            h, w = h1, w1
        return cur, h, w

    def _head(self, x, N, h, w, epi, out, out2=None, border=0, scale=1.0):
        """final 1x1 conv of a trunk output into the consumers' layouts"""
        if x.B is not None and not self._on_pc(epi):      # a head the producer / consumer kernels do not serve: materialise the merge, tiled engine
            x = self._materialise(x, N, h * w)
        self._launch(self.head, x, N, h, w, epi=epi, out=out, out2=out2, border=border, scale=scale)

    def supports_split_head(self):
        """``features_split`` is available: producer / consumer trunk and a 64 -> 64 feature head."""
        return self._on_pc(3)

    def features_split(self, x, ref_split, src_split, n_ref=1, border=2, scale=0.125, raw=False, flag=None):
        """fnet head straight into the cost volume's split-f16 operand planes (ops.feat_split's layout, csrc/cost_lines.hip): the first
        ``n_ref`` images -> ``ref_split`` [n_ref * h*w, 128] halves (plain map), the rest -> ``src_split`` [N - n_ref, (h+2b)*(w+2b), 128]
        halves whose border texels must be zero (a persistent, once-zeroed buffer).  Saves the fp32 feature maps and the feat_split pass
        (2 x 62 us and 0.67 GB of traffic at DTU size); producer / consumer engine only.  Returns (h, w)."""
        a, h, w = self._trunk_pc(x, raw)
        N = x.shape[0]
        if n_ref > 0:
            self._head(a.images(0, n_ref), n_ref, h, w, 3, ref_split, out2=flag, border=0, scale=scale)
        if N > n_ref:
            self._head(a.images(n_ref, N), N - n_ref, h, w, 3, src_split, out2=flag, border=border, scale=scale)
        return h, w

    def features(self, x, n_ref=1, border=2, scale=0.125, src_out=None, raw=False):
        """fnet head: (ref [n_ref*h*w... ] plain, src bordered).  x [N,3,H,W]; the first ``n_ref`` images go to a plain
        [n_ref, h*w, C] map, the rest to a [N-n_ref, (h+2b)*(w+2b), C] map with a zero border; both scaled."""
        a, h, w = self._trunk_pc(x, raw)
        N, C = x.shape[0], self.head.cout
        ref = torch.empty(n_ref, h * w, C, device=self.device, dtype=torch.float32)
        if n_ref > 0:
            self._head(a.images(0, n_ref), n_ref, h, w, 1, ref, border=0, scale=scale)
        src = None
        if N > n_ref:
            src = src_out if src_out is not None else torch.zeros(N - n_ref, (h + 2 * border) * (w + 2 * border), C, device=self.device,
                                                                  dtype=torch.float32)
            self._head(a.images(n_ref, N), N - n_ref, h, w, 1, src, border=border, scale=scale)
        return ref, src, h, w

    def context(self, x, raw=False):
        """cnet head: x [1,3,H,W] -> (net = tanh(first half) [P,64], inp = relu(second half) [P,64])."""
        a, h, w = self._trunk_pc(x, raw)
        half = self.head.cout // 2
        net = torch.empty(h * w, half, device=self.device, dtype=torch.float32)
        inp = torch.empty(h * w, half, device=self.device, dtype=torch.float32)
        self._head(a, 1, h, w, 2, net, out2=inp)
        return net, inp, h, w

    def forward_nchw(self, x):
        """Plain module semantics: [N,3,H,W] -> [N,Cout,h,w] (used by parity tests)."""
        a, h, w = self._trunk_pc(x, False)
        N, C = x.shape[0], self.head.cout
        out = torch.empty(N, h * w, C, device=self.device, dtype=torch.float32)
        self._head(a, N, h, w, 1, out, border=0, scale=1.0)      # (heads the producer / consumer kernels do not have - e.g. a plain 128-channel
                                                                #  output - go through the materialised merge inside _head)
        return out.view(N, h, w, C).permute(0, 3, 1, 2).contiguous()
