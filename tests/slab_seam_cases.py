"""The halo seam of the row-slab forward (cer-mvs_amd/slab.py): the shapes, the exchange loop restated with injected pieces, and the
planted faults - shared by tests/test_slab_seam_cpu.py (a 15-tap stand-in for the update iteration: proves that the harness and its faults
do what they say) and tests/test_slab_seam_gpu.py (the HIP loop).  Plain module, no fixtures.

``SHAPES``: feature-map sizes (h, w, G) with the rows every rank owns (``OWNED``, asserted from ``slab.slab_bounds`` by the CPU module):
exactly HALO owned rows (the top strip IS the bottom strip), fewer than 2 * HALO (the strips overlap), interior ranks with two halos, an
uneven split, odd widths (7 * w * 65 floats per strip half is no multiple of 4: the halves are padded), widths with and without interior
conv tiles (16 columns wide: none at w = 21, some from w = 33 on).

``slab_loop`` restates the per-iteration body of ``slab.sharded_forward`` (step -> ``pack_strips`` -> exchange -> ``unpack_halves`` or
``unpack_halo``) for G simulated ranks on ``slab.LocalExchange``; the iteration (``step``), the copy kernel (``copy``) and the row mover
of the hidden state's layout (``rows_of``) are injected.  ``fault`` plants one error.  Every fault changes VALUES only - it edits the
strips on their way from sender to receiver, or puts computed values back - and never an index range, so a planted fault cannot read or
write out of bounds on the device:

  no_disp   the disparity halo is not refreshed (the rows keep what the rank computed itself)
  short     the halo row farthest from the owned rows keeps what the rank computed itself: HALO = 6
  swapped   an interior rank receives its two halves exchanged (the upper neighbour's rows below, the lower neighbour's above).  With
            G = 2 no rank is interior: there each rank receives the OTHER half of its neighbour's buffer (the sender's halves exchanged)
  shifted   the strips hold rows r0 + 1 .. and .. r1 - 1: every strip row is its neighbour one row further inside the owned rows (the
            innermost strip row is repeated)
  late      the exchange delivers the strips of the previous iteration (zeros, what a fresh buffer holds, in the first)

``INERT``: faults that provably cannot show at a shape.  At (14, 21, 2) both extended slabs are the whole image - every row is computed
by its own rank from complete data, so rows that keep their computed values (no_disp, short) are right - and both ranks own exactly HALO
rows, so the two halves of every buffer are the same rows (swapped).  The CPU module asserts that these leave every value unchanged."""
from types import SimpleNamespace

import torch

SHAPES = ((14, 21, 2), (15, 21, 2), (22, 21, 3), (23, 50, 2), (29, 37, 3), (37, 33, 4))
OWNED = {(14, 21, 2): (7, 7), (15, 21, 2): (8, 7), (22, 21, 3): (8, 7, 7), (23, 50, 2): (12, 11), (29, 37, 3): (10, 10, 9),
         (37, 33, 4): (10, 9, 9, 9)}
FAULTS = ("no_disp", "short", "swapped", "shifted", "late")
INERT = {(14, 21, 2): ("no_disp", "short", "swapped")}
FAULT_SHAPES = ((22, 21, 3), (23, 50, 2))               # where the device module plants the faults
ONE_PER_G = ((15, 21, 2), (22, 21, 3), (37, 33, 4))     # where it runs the all-gather form
T = 3


def bounds(h, G):
    from cer_mvs_amd import slab
    return [slab.slab_bounds(h, G, g) for g in range(G)]


def seams(h, G):
    """First owned rows of ranks 1 .. G - 1."""
    return [b[0] for b in bounds(h, G)[1:]]


def rows_from_seam(rows, h, G):
    """Distance of every image row in ``rows`` to the nearest seam (0: the row below the seam; the row above it counts 1)."""
    s = seams(h, G)
    return [min(abs(r - y) if r >= y else y - r for y in s) for r in rows]


def slab_start(h, w, G, net_rows, disp, **extra):
    """The start of ``slab_loop``: per rank its bounds, its extended rows of the hidden state (``net_rows(e0, e1)``: a new tensor in the
    layout ``step`` keeps it in) and of ``disp`` [h*w] (a clone), and whatever else ``step`` needs (``extra``: name -> function of the
    rank's namespace, called once per rank)."""
    out = SimpleNamespace(h=h, w=w, G=G, slabs=[])
    for g, (r0, r1, e0, e1) in enumerate(bounds(h, G)):
        d = SimpleNamespace(g=g, r0=r0, r1=r1, e0=e0, e1=e1, hs=e1 - e0, net=net_rows(e0, e1), disp=disp[e0 * w:e1 * w].clone())
        for name, make in extra.items():
            setattr(d, name, make(d))
        out.slabs.append(d)
    return out


def _read_row(d, w, y):
    """Image row y of the rank's hidden state, flat [w * C], through the layout's row mover where there is one."""
    C = d.net.shape[1]
    if d.rows is None:
        return d.net[y * w:(y + 1) * w].reshape(-1).clone()
    flat = torch.empty(w * C, device=d.net.device, dtype=torch.float32)
    d.rows(d.net, flat, y, 1, False)
    return flat


def _shift_rows(block, halo, inward):
    """block: ``halo`` strip rows, flat.  Row j <- row j + inward (the row one further inside the owned rows), the innermost row repeated."""
    v = block.view(halo, -1)
    v.copy_(torch.cat([v[1:], v[-1:]], 0) if inward > 0 else torch.cat([v[:1], v[:-1]], 0))


def slab_loop(start, stage, G, T, exchange, step, copy, rows_of, fault=None):
    """``T`` iterations of the sharded forward's loop body from ``start`` (``slab_start``, left unchanged) -> per iteration, per rank, the
    whole extended (net, disp) after the halo refresh (clones).  ``exchange``: "p2p" (``neighbor_exchange`` + ``unpack_halves``) or
    "gather" (``all_gather_flat`` + ``unpack_halo``).  ``step(d, stage)`` advances rank namespace ``d`` (d.net, d.disp) by one iteration,
    ``copy`` is ``pack_strips``' copy, ``rows_of(hs, w)`` the row mover of an hs x w hidden state (None: plain rows)."""
    from cer_mvs_amd import slab
    assert exchange in ("p2p", "gather") and (fault is None or fault in FAULTS) and G == start.G
    w, halo = start.w, slab.HALO
    ex = slab.LocalExchange(G)
    st = []
    for s in start.slabs:
        d = SimpleNamespace(**vars(s))
        d.net, d.disp = s.net.clone(), s.disp.clone()
        d.rows = rows_of(d.hs, w)
        d.strips = torch.zeros(2 * slab.strip_half(w, d.net.shape[1]), device=d.net.device, dtype=torch.float32)
        st.append(d)
    C = st[0].net.shape[1]
    n, hb = halo * w, slab.strip_half(w, C)
    held = [torch.zeros_like(d.strips) for d in st]
    out = []
    for _ in range(T):
        send = []
        for d in st:
            step(d, stage)
            slab.pack_strips(d.net, d.disp, d.strips, w, d.r0, d.r1, d.e0, copy=copy, rows=d.rows)
            send.append(d.strips)
        # ---- faults on the strips as sent
        if fault == "shifted":
            send = [b.clone() for b in send]
            for b in send:
                for off, inward in ((0, 1), (hb, -1)):
                    _shift_rows(b[off:off + n * C], halo, inward)
                    _shift_rows(b[off + n * C:off + n * C + n], halo, inward)
        if fault == "late":
            send, held = held, [b.clone() for b in send]
        if fault == "swapped" and G == 2:
            send = [torch.cat([b[hb:], b[:hb]]) for b in send]
        # ---- exchange (the receive buffers are cloned where a fault edits them: LocalExchange hands out shared storage)
        if exchange == "p2p":
            halves = [tuple(None if x is None else x.clone() for x in pair) for pair in ex.neighbor_exchange(send)]
        else:
            flat = [f.clone() for f in ex.all_gather_flat(send)]
            halves = [(flat[g][g - 1][hb:] if g > 0 else None, flat[g][g + 1][:hb] if g < G - 1 else None) for g in range(G)]
        for g, d in enumerate(st):
            prev_half, next_half = halves[g]
            # ---- faults on the strips as received (in place: in the gather form the halves are views of ``flat[g]``)
            if fault == "swapped" and prev_half is not None and next_half is not None:
                keep = prev_half.clone()
                prev_half.copy_(next_half)
                next_half.copy_(keep)
            if fault == "short":
                if prev_half is not None and d.r0 - d.e0 == halo:
                    prev_half[:w * C] = _read_row(d, w, 0)
                    prev_half[n * C:n * C + w] = d.disp[:w]
                if next_half is not None and d.e1 - d.r1 == halo:
                    prev_row = d.hs - 1
                    next_half[(halo - 1) * w * C:n * C] = _read_row(d, w, prev_row)
                    next_half[n * C + n - w:n * C + n] = d.disp[prev_row * w:]
            own_disp = d.disp.clone() if fault == "no_disp" else None
            if exchange == "p2p":
                slab.unpack_halves(d.net, d.disp, prev_half, next_half, w, g, G, d.r0, d.r1, d.e0, d.e1, copy=copy, rows=d.rows)
            else:
                slab.unpack_halo(d.net, d.disp, flat[g], w, g, G, d.r0, d.r1, d.e0, d.e1, copy=copy, rows=d.rows)
            if own_disp is not None:
                d.disp[:(d.r0 - d.e0) * w] = own_disp[:(d.r0 - d.e0) * w]
                d.disp[(d.r1 - d.e0) * w:] = own_disp[(d.r1 - d.e0) * w:]
        out.append([(d.net.clone(), d.disp.clone()) for d in st])
    return out
