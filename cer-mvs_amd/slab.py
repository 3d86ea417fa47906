"""Spatially sharded depth inference across the GPUs of one node.

Rank g of G
  * encodes the reference view, the context map and ITS source views (views v with (v-1) % G == g) and all-gathers the
    source feature maps (the exchange step of the cost volume - RCCL all-gather over xGMI);
  * owns a slab of image rows: builds the view-summed cost volume for its rows (all V views - no all-reduce needed) and runs
    the GRU loop on the slab extended by HALO rows on each interior side;
  * after every iteration all-gathers the HALO owned rows next to each slab border of (net, disp) and refreshes its halo.
HALO = 7 is the receptive-field growth of one update-block iteration (corr_encoder 3x3: 1 row; z|r: 7x7 unfold + 3x3 = 4;
q: 5; delta head two 3x3: 7): rows closer than 7 to an interior slab edge are computed from zero padding instead of the
neighbour's data, are never used, and are overwritten by the next refresh.  Results equal the single-GPU forward.

The collective layer is injectable: ``DistExchange`` (torch.distributed, one rank per process) or ``LocalExchange`` (G
simulated ranks in one process - used to validate the slab logic on a single GPU and on CPU)."""
import torch

HALO = 7


def slab_bounds(h, G, g, halo=HALO):
    """Owned rows [r0, r1) and extended rows [e0, e1) of rank g (balanced split, remainder to the first ranks)."""
    base, rem = divmod(h, G)
    r0 = g * base + min(g, rem)
    r1 = r0 + base + (1 if g < rem else 0)
    return r0, r1, max(r0 - halo, 0), min(r1 + halo, h)


def can_shard(h, G, halo=HALO):
    """Every rank must own at least ``halo`` rows (its border strip is what the neighbour's halo is refreshed from)."""
    return h // G >= halo


class LocalExchange:
    """G simulated ranks in one process: all_gather(list of G tensors) -> each rank sees the whole list."""

    def __init__(self, G):
        self.G = G
        self.ranks = list(range(G))

    def all_gather(self, tensors):
        assert len(tensors) == self.G
        return [list(tensors) for _ in range(self.G)]

    def all_gather_async(self, tensors):
        return self.all_gather(tensors)

    def wait(self, handle):
        return handle

    def gather_flat_async(self, tensors, tag="f"):
        """Start gathering every rank's tensor into ONE persistent [G, ...] buffer; ``wait_flat`` returns it per local rank."""
        t = tensors[0]
        key = (tag, tuple(t.shape), t.device, t.dtype)
        bufs = getattr(self, "_gf", None)
        if bufs is None:
            bufs = self._gf = {}
        if key not in bufs:
            bufs[key] = torch.empty((self.G,) + tuple(t.shape), device=t.device, dtype=t.dtype)
        out = bufs[key]
        for g, x in enumerate(tensors):
            out[g].copy_(x)
        return out

    def wait_flat(self, handle):
        return [handle for _ in range(self.G)]

    def neighbor_exchange(self, bufs):
        """Simulated point-to-point halo refresh: rank g sees the bottom half of g-1's buffer and the top half of g+1's
        (copies, like the real receive buffers)."""
        half = bufs[0].numel() // 2
        key = (bufs[0].numel(), bufs[0].device, bufs[0].dtype)
        if getattr(self, "_nb_key", None) != key:      # persistent receive buffers, like DistExchange: recorded launches point into them
            self._nb_key = key
            self._nb = [(torch.empty(half, device=bufs[0].device, dtype=bufs[0].dtype), torch.empty(half, device=bufs[0].device, dtype=bufs[0].dtype))
                        for _ in range(self.G)]
        out = []
        for g in range(self.G):
            rp, rn = self._nb[g]
            if g > 0:
                rp.copy_(bufs[g - 1][half:])
            if g < self.G - 1:
                rn.copy_(bufs[g + 1][:half])
            out.append((rp if g > 0 else None, rn if g < self.G - 1 else None))
        return out

    def max_int(self, value, device):
        """MAX of a host integer over the ranks (all of them live in this process)."""
        return int(value)

    def all_gather_flat(self, tensors):
        """list of G equal-sized tensors -> per simulated rank the stacked [G, ...] tensor."""
        assert len(tensors) == self.G
        t = tensors[0]
        key = (tuple(t.shape), t.device, t.dtype)
        if getattr(self, "_flat_key", None) != key:      # persistent, like DistExchange: recorded launches point into it
            self._flat_key, self._flat = key, torch.empty((self.G,) + tuple(t.shape), device=t.device, dtype=t.dtype)
        torch.stack(list(tensors), 0, out=self._flat)
        return [self._flat for _ in range(self.G)]


class DistExchange:
    """One rank per process on a torch.distributed group (backend nccl = RCCL over xGMI on the GPU box, gloo in CPU tests)."""

    def __init__(self, group=None):
        import torch.distributed as dist
        self.group = group
        self.G = dist.get_world_size(group)
        self.ranks = [dist.get_rank(group)]

    def max_int(self, value, device):
        """MAX of a host integer over the ranks (one tiny all-reduce; used for the overflow flag under overflow_policy="raise")."""
        import torch.distributed as dist
        on_dev = dist.get_backend(self.group) == "nccl"
        t = torch.tensor([int(value)], dtype=torch.int32, device=device if on_dev else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.group)
        return int(t.item())

    def neighbor_exchange(self, bufs):
        """Halo refresh as point-to-point traffic: this rank's buffer is [top half | bottom half]; the top half goes to rank g-1,
        the bottom half to rank g+1, and their facing halves come back - 2 sends + 2 receives of one strip each
        (``batch_isend_irecv``: one RCCL group call, neighbour links of the xGMI mesh only) instead of an all-gather in which every
        rank receives all G buffers.  Returns [(prev_half or None, next_half or None)] (persistent receive buffers)."""
        import torch.distributed as dist
        buf = bufs[0]
        g, G = self.ranks[0], self.G
        half = buf.numel() // 2
        key = (buf.data_ptr(), buf.numel(), buf.device, buf.dtype)
        if getattr(self, "_nb_key", None) != key:
            # persistent receive buffers and - the send buffer is persistent too - the P2P op list, built once per forward
            self._nb_key = key
            self._nb = (torch.empty(half, device=buf.device, dtype=buf.dtype), torch.empty(half, device=buf.device, dtype=buf.dtype))
            ranks = dist.get_process_group_ranks(self.group) if self.group is not None else list(range(G))
            # RCCL orders the transfers after the launch stream's kernels by itself.  gloo (the transport of the multi-process tests)
            # has no stream semantics for point-to-point device buffers: there the strips are staged through host tensors.
            self._nb_staged = buf.is_cuda and dist.get_backend(self.group) != "nccl"
            if self._nb_staged:
                self._nb_host = (torch.empty(buf.numel(), dtype=buf.dtype), torch.empty(half, dtype=buf.dtype), torch.empty(half, dtype=buf.dtype))
                src, dprev, dnext = self._nb_host
            else:
                src, (dprev, dnext) = buf, self._nb
            ops_ = []
            if g > 0:
                ops_ += [dist.P2POp(dist.isend, src[:half], ranks[g - 1], self.group), dist.P2POp(dist.irecv, dprev, ranks[g - 1], self.group)]
            if g < G - 1:
                ops_ += [dist.P2POp(dist.isend, src[half:], ranks[g + 1], self.group), dist.P2POp(dist.irecv, dnext, ranks[g + 1], self.group)]
            self._nb_ops = ops_
        rprev, rnext = self._nb
        if self._nb_staged:
            self._nb_host[0].copy_(buf)
        for w_ in (dist.batch_isend_irecv(self._nb_ops) if self._nb_ops else []):
            w_.wait()
        if self._nb_staged:
            if g > 0:
                rprev.copy_(self._nb_host[1])
            if g < G - 1:
                rnext.copy_(self._nb_host[2])
        return [(rprev if g > 0 else None, rnext if g < G - 1 else None)]

    def all_gather(self, tensors):
        import torch.distributed as dist
        t = tensors[0].contiguous()
        out = [torch.empty_like(t) for _ in range(self.G)]
        dist.all_gather(out, t, group=self.group)
        return [out]

    def all_gather_async(self, tensors):
        """Start an all-gather; ``wait`` returns what ``all_gather`` would (the collective runs on RCCL's own stream meanwhile)."""
        import torch.distributed as dist
        t = tensors[0].contiguous()
        out = [torch.empty_like(t) for _ in range(self.G)]
        return dist.all_gather(out, t, group=self.group, async_op=True), out, t

    def wait(self, handle):
        handle[0].wait()
        return [handle[1]]

    def gather_flat_async(self, tensors, tag="f"):
        """Start an all-gather of this rank's tensor into ONE persistent [G, ...] buffer (no per-call allocations, nothing to
        reassemble afterwards); the collective runs on RCCL's own stream until ``wait_flat``."""
        import torch.distributed as dist
        t = tensors[0]
        key = (tag, tuple(t.shape), t.device, t.dtype)
        bufs = getattr(self, "_gf", None)
        if bufs is None:
            bufs = self._gf = {}
        if key not in bufs:
            bufs[key] = torch.empty((self.G,) + tuple(t.shape), device=t.device, dtype=t.dtype)
        out = bufs[key]
        if dist.get_backend(self.group) == "nccl":
            work = dist.all_gather_into_tensor(out, t, group=self.group, async_op=True)
        else:
            work = dist.all_gather(list(out.unbind(0)), t, group=self.group, async_op=True)
        return work, out, t

    def wait_flat(self, handle):
        handle[0].wait()
        return [handle[1]]

    def all_gather_flat(self, tensors):
        """One collective into one preallocated [G, ...] buffer (no per-rank output tensors, no copies after it)."""
        import torch.distributed as dist
        t = tensors[0]
        key = (tuple(t.shape), t.device, t.dtype)
        if getattr(self, "_flat_key", None) != key:
            self._flat_key, self._flat = key, torch.empty((self.G,) + tuple(t.shape), device=t.device, dtype=t.dtype)
        out = self._flat
        if dist.get_backend(self.group) == "nccl":
            dist.all_gather_into_tensor(out, t, group=self.group)
        else:
            dist.all_gather(list(out.unbind(0)), t, group=self.group)
        return [out]


def border_strips(x, w, r0, r1, e0, halo=HALO):
    """x [rows_ext*w, C] -> [2, halo*w, C]: the first and last ``halo`` OWNED rows (what the neighbours need)."""
    top = x[(r0 - e0) * w:(r0 - e0 + halo) * w]
    bot = x[(r1 - halo - e0) * w:(r1 - e0) * w]
    return torch.stack([top, bot], 0)


def refresh_halo(x, strips, w, g, G, r0, r1, e0, e1, halo=HALO):
    """Fill the halo rows of x [rows_ext*w, C] from the neighbours' strips (list indexed by rank, each [2, halo*w, C])."""
    if g > 0 and r0 > e0:          # rows [e0, r0) = the last `halo` owned rows of rank g-1
        x[:(r0 - e0) * w] = strips[g - 1][1][(halo - (r0 - e0)) * w:]
    if g < G - 1 and e1 > r1:      # rows [r1, e1) = the first `halo` owned rows of rank g+1
        x[(r1 - e0) * w:] = strips[g + 1][0][:(e1 - r1) * w]
    return x


def _device_copy(pairs):
    from . import ops
    ops.copy_segments(pairs)


def strip_half(w, C, halo=HALO):
    """Floats per half of a strips buffer: ``halo`` rows of net (C channels) + of disp, rounded up to a multiple of 4 so that the
    second half - and with it the net rows the 16-byte row mover writes - starts 16-byte aligned for any image width."""
    return (halo * w * (C + 1) + 3) // 4 * 4


def pack_strips(net, disp, buf, w, r0, r1, e0, halo=HALO, copy=_device_copy, rows=None):
    """The first / last ``halo`` OWNED rows of net [rows_ext*w, C] and disp [rows_ext*w] -> buf, laid out as two halves
    [net top | disp top] [net bottom | disp bottom] (the top half is what rank g-1 needs, the bottom half what g+1 needs).
    All four ranges are contiguous: one cer_copy_segments_f32 launch.
    ``rows(net, flat, y0, nrows, to_tensor)``: row mover for a hidden state kept in an m-tile-major layout (s16 path)."""
    C = net.shape[1]
    n, t0, b0 = halo * w, (r0 - e0) * w, (r1 - halo - e0) * w
    hb = strip_half(w, C, halo)
    if rows is not None:
        rows(net, buf[:n * C], r0 - e0, halo, False)
        rows(net, buf[hb:hb + n * C], r1 - halo - e0, halo, False)
        copy([(disp[t0:t0 + n], buf[n * C:n * C + n]), (disp[b0:b0 + n], buf[hb + n * C:hb + n * C + n])])
        return
    copy([(net[t0:t0 + n], buf[:n * C]), (disp[t0:t0 + n], buf[n * C:n * C + n]),
          (net[b0:b0 + n], buf[hb:hb + n * C]), (disp[b0:b0 + n], buf[hb + n * C:hb + n * C + n])])


def unpack_halves(net, disp, prev_half, next_half, w, g, G, r0, r1, e0, e1, halo=HALO, copy=_device_copy, rows=None):
    """Refresh the halo rows of (net, disp): rows [e0, r0) from ``prev_half`` = the BOTTOM half of rank g-1's strips buffer (its
    last ``halo`` owned rows), rows [r1, e1) from ``next_half`` = the TOP half of rank g+1's; layout of pack_strips.  One launch
    (plus the row mover's, s16 path)."""
    C = net.shape[1]
    n = halo * w
    pairs = []
    if g > 0 and r0 > e0:          # rows [e0, r0) = the last (r0-e0) rows of rank g-1's bottom strip
        k = (r0 - e0) * w
        if rows is not None:
            rows(net, prev_half[(n - k) * C:n * C], 0, r0 - e0, True)
        else:
            pairs += [(prev_half[(n - k) * C:n * C], net[:k])]
        pairs += [(prev_half[n * C + (n - k):n * C + n], disp[:k])]
    if g < G - 1 and e1 > r1:      # rows [r1, e1) = the first (e1-r1) rows of rank g+1's top strip
        k, o = (e1 - r1) * w, (r1 - e0) * w
        if rows is not None:
            rows(net, next_half[:k * C], r1 - e0, e1 - r1, True)
        else:
            pairs += [(next_half[:k * C], net[o:o + k])]
        pairs += [(next_half[n * C:n * C + k], disp[o:o + k])]
    if pairs:
        copy(pairs)


def unpack_halo(net, disp, allbuf, w, g, G, r0, r1, e0, e1, halo=HALO, copy=_device_copy, rows=None):
    """``unpack_halves`` on the gathered strips allbuf [G, 2 * strip_half] of the all-gather form of the exchange."""
    hb = strip_half(w, net.shape[1], halo)
    unpack_halves(net, disp, allbuf[g - 1][hb:] if g > 0 else None, allbuf[g + 1][:hb] if g < G - 1 else None, w, g, G, r0, r1, e0, e1,
                  halo, copy, rows)


P2P_HALO = True           # halo refresh by neighbour point-to-point exchange (False: one all-gather of every rank's strips)


def _finish_overflow(model, ex, dev):
    """End-of-forward overflow handling of the sharded path.  "lazy": asynchronous snapshot, polled by the next forward (every rank
    polls its own flag; the ranks run the same GRU on overlapping rows, but a rank can saturate alone - a hit then raises on that
    rank at its next forward).  "raise": the flag is read here and MAX-reduced over the ranks, so that every rank raises together
    instead of one rank leaving the collective sequence.  "fallback" has no sharded form: it is refused up front (sharded_forward)."""
    from . import ops
    policy = getattr(model, "overflow_policy", "lazy")
    if policy == "lazy":
        ops.overflow_snapshot(dev)
    elif policy == "raise":
        bits = ex.max_int(int(ops.check_overflow(dev)), dev)
        if bits:
            model._raise_overflow(bits)


def sharded_forward(model, images, poses, intrinsics, scale, ex):
    """Test-mode RAFT.forward sharded over ``ex.G`` ranks; ``ex.ranks`` are the ranks simulated by this process.
    Returns the full-resolution disparity [1,1,h,w] * scale (identical on every rank)."""
    from . import _lib as L, ops, update
    from .dist import local_views_for
    from .projective import pij_matrices, scaled_cameras
    dev = images.device
    G = ex.G
    if getattr(model, "overflow_policy", "lazy") == "fallback":
        raise NotImplementedError("RAFT.overflow_policy='fallback' is not available on the sharded forward (every rank would have to "
                                  "repeat the forward together): use 'lazy' or 'raise'")
    factor = 8 if model.encoder_type == "LR" else 4
    poses, intr, s = scaled_cameras(poses, intrinsics, scale, factor)
    _, num, _, ht, wd = images.shape
    if ht % factor or wd % factor:
        raise RuntimeError(f"sharded_forward: image size {wd}x{ht} must be a multiple of {factor}")
    images = images.float()                               # (normalised inside the encoders' stem kernel)
    h, w = ht // factor, wd // factor
    V = num - 1
    ub = model.update_block
    C = model.dim_fmap
    vmax = (V + G - 1) // G
    Pb = (h + 4) * (w + 4)

    # (uploaded before anything is enqueued: a pageable H2D copy blocks the host until the stream has drained)
    Pij = pij_matrices(poses[0], intr[0], [0] * V, list(range(1, V + 1))).to(dev)

    # ---- encoders: each rank its own source views first, so that their all-gather (333 MB at 1600x1184 x 10 views: the exchange
    # step of the cost volume) is in flight while the rank encodes the reference view and the context map
    st = {}
    send = []
    # cost volume on the epipolar-line-tile kernel (C = 64, D <= 64): every rank splits ITS views' rows to f16 hi|lo (same bytes)
    # and the all-gather lands them in one persistent [G, vmax, Pb, 128] buffer that the kernel reads through a view -> block map -
    # no per-view reassembly copies, no fresh 333 MB buffer per forward.  Otherwise (fp32 walk): gather fp32 rows and reorder.
    lines = all(ops.on_line_tiles(C, D) for D, _, _ in model.stages())
    pads = getattr(model, "_slab_pads", None)
    if pads is None:
        pads = model._slab_pads = {}
    for g in ex.ranks:
        views = local_views_for(V, G, g)
        _, _, _, f2 = model.encode(images, views, raw=True, parts="src")
        key = (g, vmax, Pb, lines, str(dev))
        pad = pads.get(key)
        if pad is None:                                   # persistent; rows of unused view slots stay zero
            pad = pads[key] = torch.zeros(vmax, Pb, 128 if lines else C, device=dev, dtype=torch.float16 if lines else torch.float32)
        if views:
            if lines:
                ops.feat_split(f2, out=pad[:len(views)])
            else:
                pad[:len(views)] = f2
        send.append(pad)
    pending = ex.gather_flat_async(send, tag="f2")
    for g in ex.ranks:
        net_l, inp_l, f1, _ = model.encode(images, [], raw=True, parts="ref")
        st[g] = dict(net=net_l, inp=inp_l, f1=f1)
    gathered = ex.wait_flat(pending)
    # view v (1-based) lives with rank (v-1) % G in that rank's slot (v-1) // G
    slots = torch.tensor([((v - 1) % G) * vmax + (v - 1) // G for v in range(1, V + 1)], dtype=torch.int32)
    for i, g in enumerate(ex.ranks):
        if lines:
            st[g]["f2"] = None
            st[g]["f2s"] = gathered[i]
            st[g]["slots"] = slots.to(dev)
        else:
            st[g]["f2"] = gathered[i].view(G * vmax, Pb, C).index_select(0, slots.to(dev).long())

    # ---- slabs
    for g in ex.ranks:
        r0, r1, e0, e1 = slab_bounds(h, G, g)
        d = st[g]
        d.update(r0=r0, r1=r1, e0=e0, e1=e1, hs=e1 - e0)
        d["net"] = ub.prepare_net(d["net"][e0 * w:e1 * w].clone(), e1 - e0, w)
        d["inp"] = d["inp"][e0 * w:e1 * w].contiguous()
        d["f1s"] = d["f1"][e0 * w:e1 * w].contiguous()
        d["split"] = (ops.feat_split(d["f1s"]), d["f2s"], d["slots"]) if lines else None
        d["disp"] = torch.zeros((e1 - e0) * w, device=dev, dtype=torch.float32)
        d["hoist"] = ub.hoist_all(d["inp"], e1 - e0, w, len(model.cascade))
        d["ws"] = ub.workspace(e1 - e0, w, dev)
        d["strips"] = torch.zeros(2 * strip_half(w, d["net"].shape[1]), device=dev, dtype=torch.float32)
        d["rows"] = ub.loop(0, dev).rows(e1 - e0, w)      # (s16 path: the hidden state's image rows move through cer_s16_rows_f32)

    for stage, (D, incre, T) in enumerate(model.stages()):
        for g in ex.ranks:
            d = st[g]
            vol, origin = ops.cost_build(d["f1s"], d["f2"], Pij, d["disp"], D, incre, stage == 0, d["hs"], w, ub.num_levels,
                                         fold=True, src_hw=(h, w), y0=d["e0"], pyramid_scale=(1.0 / V) if D <= 64 else None,
                                         split=d["split"], compact=True, two_term=model._cost_x2)
            if D > 64:
                ops.pyramid(vol, D, 1, scale=1.0 / V)        # (level-0-only rows, as in RAFT._run_stages)
            d["vol"], d["origin"] = vol, origin
        loop = ub.loop(stage, dev)             # host-side weight packing stays out of the recorded plans
        for it in range(T):
            record = it == 0 or not update.USE_PLANS
            send = []
            for g in ex.ranks:
                d = st[g]
                if record:
                    # iteration + pack of the 2 x HALO border rows of (net, disp): recorded once per stage, then replayed
                    d["plan_step"] = L.LaunchPlan(keep=(d["vol"], d["origin"]))
                    with L.recording(d["plan_step"]):
                        loop.step(d["vol"], d["origin"], d["net"], d["disp"], d["hoist"][stage], d["hs"], w, D, incre, d["ws"])
                        pack_strips(d["net"], d["disp"], d["strips"], w, d["r0"], d["r1"], d["e0"], rows=d["rows"])
                else:
                    d["plan_step"].replay()
                send.append(d["strips"])
            if P2P_HALO:                          # neighbours only: 2 sends + 2 receives of one strip per rank
                halves = ex.neighbor_exchange(send)
            else:                                 # one collective: every rank receives all G strip buffers
                gathered = ex.all_gather_flat(send)
                hb = send[0].numel() // 2
                halves = [(gathered[i][g - 1][hb:] if g > 0 else None, gathered[i][g + 1][:hb] if g < G - 1 else None)
                          for i, g in enumerate(ex.ranks)]
            for i, g in enumerate(ex.ranks):
                d = st[g]
                if record:
                    d["plan_halo"] = L.LaunchPlan(keep=(halves[i],))
                    with L.recording(d["plan_halo"]):
                        unpack_halves(d["net"], d["disp"], halves[i][0], halves[i][1], w, g, G, d["r0"], d["r1"], d["e0"], d["e1"],
                                      rows=d["rows"])
                else:
                    d["plan_halo"].replay()
        if T > 0:                                 # what UpdateBlock.run does after a stage's last iteration, with THIS stage's loop
            for g in ex.ranks:
                loop.finish(st[g]["ws"])

    # ---- saturation is never silent on the sharded path either: every bit was or-ed into the flag by the kernels
    # themselves (the slab loop calls step, not UpdateBlock.run: the loop's own end-of-stage step ran per stage above)
    _finish_overflow(model, ex, dev)

    # ---- gather the owned rows of every rank (persistent send / receive buffers)
    rows_max = (h + G - 1) // G
    send = []
    owns = getattr(model, "_slab_own", None)
    if owns is None:
        owns = model._slab_own = {}
    for g in ex.ranks:
        d = st[g]
        key = (g, rows_max * w, str(dev))
        own = owns.get(key)
        if own is None:
            own = owns[key] = torch.zeros(rows_max * w, device=dev, dtype=torch.float32)
        n = (d["r1"] - d["r0"]) * w
        own[:n] = d["disp"][(d["r0"] - d["e0"]) * w:(d["r1"] - d["e0"]) * w]
        send.append(own)
    gathered = ex.wait_flat(ex.gather_flat_async(send, tag="disp"))
    if h % G == 0:                                        # equal slabs: the gathered buffer IS the disparity map
        return gathered[0].reshape(1, 1, h, w) * s
    out = torch.empty(h * w, device=dev, dtype=torch.float32)
    for r in range(G):
        r0, r1, _, _ = slab_bounds(h, G, r)
        out[r0 * w:r1 * w] = gathered[0][r][:(r1 - r0) * w]
    return out.view(1, 1, h, w) * s
