"""Cloud-to-cloud evaluation on the device (csrc/cloud_eval.hip): the exact nearest neighbour of every point of one cloud in
another within a cut-off, and the two published protocols built on it - DTU's accuracy / completeness / overall (means of those distances)
and Tanks-and-Temples' precision / recall / F-score (shares of them below a threshold).

    from cer_mvs_amd.cloud_eval import accuracy_completeness, fscore
    out = reconstruct_scan(model, ..., write=False)
    pred = torch.from_numpy(out["xyz"]).cuda()
    accuracy_completeness(pred, gt, max_dist=20.0, thin=0.2)      # {"accuracy", "completeness", "overall", "n_pred", ...}
    accuracy_completeness(pred, gt, max_dist=20.0, thin=0.2, thin_method="greedy")      # DTU's own reduction of pred (radius_thin)
    fscore(pred, gt, tau=0.01)                                    # {"precision", "recall", "fscore", ...}

Clouds are CUDA float32 tensors [n, 3]; there is no CPU fallback.  Sorting (``torch.sort(stable=True)``) and the reductions over the distance
vector (fp64 ``sum`` / ``count_nonzero``) are torch; keys, the cell table, the record gather and the search are HIP kernels.  Everything is a
pure function of its inputs: no atomics, the same bytes on every run.  Reading ground-truth files, crop volumes, observability masks and
ground planes of the benchmarks is the caller's business (``keep_pred`` / ``keep_gt`` carry masks in).

Clouds in slightly different frames are registered first (csrc/cloud_align.hip): point-to-point ICP on the same search,

    T = register(pred, gt, stages=((4 * tau, 8 * tau, 30), (None, 3 * tau, 30)))["T"]      # coarse to fine; or icp(pred, gt, max_dist)
    fscore(pred, gt, tau, align=T)

with ``rigid_transform`` and ``pair_moments`` as its two kernels and ``rigid_from_moments`` (Kabsch, numpy fp64) as its solve.  On a surface,
point-to-plane ICP needs a fraction of the iterations - the target's normals let a match slide along the surface:

    icp(pred, gt, max_dist, method="plane")                       # normals of gt estimated once (or dst_normals=...); register(...) likewise

with ``plane_moments`` (the 6x6 normal equations, 30 fp64 sums in the same tree) and ``rigid_from_plane_moments`` as kernel and solve.

The same index answers two more queries: ``CloudIndex.knn`` / ``knn_mean_distance`` - the k <= 32 nearest points of every query
in ascending (d2, index) order, or only their mean distance - and ``CloudIndex.count_within``, the number of points within a radius; same
contract: fp64 distances, lowest index on ties, inclusive cut-off, no atomics.  The two standard outlier filters for fused clouds rest on them:

    keep = remove_statistical_outliers(pred, k=20, std_ratio=2.0)      # or remove_radius_outliers(pred, radius, min_neighbours)
    pred = pred.index_select(0, keep)
    reconstruct_scan(model, ..., clean={"method": "statistical", "k": 20, "std_ratio": 2.0})      # the same, before the cloud leaves the device

... and a third: ``CloudIndex.normals`` / ``estimate_normals`` - the surface normal and the curvature (surface variation) at every
point, from the plane through its k nearest neighbours (the eigenvectors of their fp64 covariance, found in the search kernel's registers), turned
towards a viewpoint when there is one - what a mesher or a relighter asks of a cloud:

    normal, curvature = estimate_normals(pred, k=20, viewpoints=camera_centre)      # float32 [n, 3] (zeros where there is no plane), float32 [n]
    reconstruct_scan(model, ..., normals=True)      # every point turned towards the camera that produced it; result.ply carries nx ny nz"""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L

GRID_TILE = 2048                                             # cer_mvs.h CER_GRID_TILE
GRID_COORD_LIMIT = 1 << 20                                   # cer_mvs.h CER_GRID_COORD_LIMIT
GRID_MAX_RINGS = 4096                                        # cloud_eval.hip GRID_MAX_RINGS: ceil(reach / cell) beyond this is refused
# cloud_distances' default cell is max_dist / DEFAULT_CELL_DIVISOR.  The search cuts every row of cells to what can still beat the best
# distance so far, so its work follows the distance to the neighbour, not max_dist; the cell size sets how many points come along with the
# neighbour (one cell's worth at least) against how many cells an empty query must look up ((2 * divisor + 3)^2 rows).  Measured by
# tools/bench_cloud_eval.py (profiles/cloud_eval_bench.json "cell_sweep").
DEFAULT_CELL_DIVISOR = 4
# radius_thin runs this many rounds between two compactions of its active list (each compaction costs three small launches and the one
# host read that tells the loop whether anything is left).  Measured by tools/bench_cloud_thin.py against 1 and 4
# (profiles/cloud_thin_bench.json "rounds_per_compaction").
THIN_ROUNDS_PER_COMPACTION = 2
KNN_MAX = 32                                                 # cer_mvs.h CER_KNN_MAX: the widest neighbour list the search keeps in registers
# The outlier filters' default cell is max_dist (or radius) / this.  Twenty neighbours reach farther than one, so the divisor measured for
# ``nearest`` need not have held: tools/bench_cloud_knn.py sweeps 1, 2, 4, 8 at k = 20, and 4 wins there too (profiles/cloud_knn_bench.json
# "cell_sweep").
KNN_CELL_DIVISOR = DEFAULT_CELL_DIVISOR
MOMENT_TILE = 2048                                           # cer_mvs.h CER_MOMENT_TILE
MOMENT_COUNT = 17                                            # cer_mvs.h CER_MOMENT_COUNT
COLLINEAR_RATIO = 1e-12                                      # rigid_from_moments: second singular value / first at or below this -> no rotation
PLANE_MOMENT_COUNT = 30                                      # cer_mvs.h CER_PLANE_MOMENT_COUNT
PLANE_DEGENERATE = 1e-10                                     # rigid_from_plane_moments: smallest eigenvalue of the scaled normal matrix at or below this -> no step
NORMAL_DEGENERATE = COLLINEAR_RATIO                       # cloud_eval.hip NORMAL_DEGENERATE: second eigenvalue / largest at or below this -> no normal


def _cloud(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor (no CPU fallback)")
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{name}: points [n, 3] expected")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32")
    if t.shape[0] >= 1 << 31:
        raise ValueError(f"{name}: fewer than 2^31 points expected")
    return t.contiguous()


def _cell(cell):
    cell = float(cell)
    if not (cell > 0.0 and math.isfinite(cell)):
        raise ValueError("cell must be a positive finite number")
    return cell


def _knn_k(k):
    k = int(k)
    if not 1 <= k <= KNN_MAX:
        raise ValueError(f"k: 1 .. {KNN_MAX} expected, got {k}")
    return k


def _reach(value, name, finite=False):
    """a search's reach (``max_dist``, ``radius``) as the float32 the kernels take: >= 0 (+inf allowed unless ``finite``), ValueError otherwise"""
    value = float(np.float32(value))
    if not (value >= 0.0 and (math.isfinite(value) or not finite)):
        raise ValueError(f"{name} must be {'a finite number ' if finite else ''}>= 0")
    return value


class CloudIndex:
    """Sparse uniform grid over ``points`` (CUDA float32 [n, 3]) with cell edge ``cell``: keys, one stable sort and the cell table, built once.
    The grid's origin is the per-axis minimum of the finite points, promoted to fp64.  ``n``: the indexed (finite) points; points with a NaN
    or infinite coordinate are never anybody's neighbour.  ``order``: original indices in sorted order (int64 [n_all]); ``cell_start``: first
    sorted position of every occupied cell, int64 [cells + 1]."""

    def __init__(self, points, cell):
        points = _cloud(points, "points")
        self.cell = _cell(cell)
        self.points = points
        dev = points.device
        n_all = int(points.shape[0])
        lib = L.load()
        self.origin = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
        self.n, self.cells = 0, 0
        self.records = self.cell_keys = None
        self.order = torch.empty(0, device=dev, dtype=torch.int64)
        self.cell_start = torch.zeros(1, device=dev, dtype=torch.int64)
        if n_all == 0:
            return
        finite = torch.isfinite(points).all(1, keepdim=True)
        lo = torch.where(finite, points, points.new_full((), float("inf"))).amin(0).double().cpu()      # (read 1: the origin travels as an argument)
        if not bool(torch.isfinite(lo).all()):
            self.order = torch.arange(n_all, device=dev)
            return                                           # no finite point: an empty index
        self.origin = (ctypes.c_double * 3)(*[float(v) for v in lo])
        keys = torch.empty(n_all, device=dev, dtype=torch.int64)
        flag = torch.empty(1, device=dev, dtype=torch.int32)
        rc = lib.cer_grid_keys_f32(L.dev_ptr(points, "points"), n_all, self.origin, self.cell, 0, L.dev_ptr(keys, "keys", torch.int64),
                                   L.dev_ptr(flag, "flag", torch.int32), L.cur_stream())
        if rc == -2:
            raise ValueError(f"CloudIndex: the cloud spans more than 2^20 cells of {self.cell} along an axis; use a larger cell")
        L.check(rc, "grid_keys")
        keys, self.order = torch.sort(keys, stable=True)
        partials, offsets, totals = L.compaction_buffers(int(lib.cer_grid_partials(n_all)), dev, extra=1)
        pk = L.dev_ptr(keys, "keys", torch.int64)
        L.check(lib.cer_grid_cells_count_i64(pk, n_all, L.dev_ptr(partials, "partials", torch.int32), L.dev_ptr(offsets, "offsets", torch.int64),
                                             L.dev_ptr(totals, "totals", torch.int64), L.cur_stream()), "grid_cells_count")
        self.cells, self.n = (int(v) for v in totals.cpu())                                              # (read 2: sizes the cell table)
        self.cell_keys = torch.empty(self.cells, device=dev, dtype=torch.int64)
        self.cell_start = torch.empty(self.cells + 1, device=dev, dtype=torch.int64)
        L.check(lib.cer_grid_cells_i64(pk, n_all, L.dev_ptr(offsets, "offsets", torch.int64), self.cells,
                                       L.dev_ptr(self.cell_keys, "cell_keys", torch.int64), L.dev_ptr(self.cell_start, "cell_start", torch.int64),
                                       L.cur_stream()), "grid_cells")
        self.records = torch.empty(n_all, 4, device=dev, dtype=torch.int32)
        L.check(lib.cer_grid_pack_f32(L.dev_ptr(points, "points"), L.dev_ptr(self.order, "order", torch.int64), n_all,
                                      L.dev_ptr(self.records, "records", torch.int32), L.cur_stream()), "grid_pack")

    def grid_args(self):                                     # the argument head of both searches, cer_grid_nearest_f32's first seven
        return (L.dev_ptr(self.records, "records", torch.int32), self.n, L.dev_ptr(self.cell_keys, "cell_keys", torch.int64),
                L.dev_ptr(self.cell_start, "cell_start", torch.int64), self.cells, self.origin, self.cell)

    def heads(self):
        """Original index of the first sorted point of every occupied cell - the lowest index in the cell, as the sort is stable."""
        return self.order[self.cell_start[:self.cells]]

    def _walk_order(self, queries, m):                       # the queries' positions in the order of their own cell keys
        qkeys = torch.empty(m, device=queries.device, dtype=torch.int64)
        L.check(L.load().cer_grid_keys_f32(L.dev_ptr(queries, "queries"), m, self.origin, self.cell, 1, L.dev_ptr(qkeys, "keys", torch.int64), None,
                                           L.cur_stream()), "grid_keys")
        return torch.sort(qkeys, stable=True).indices

    def _query(self, method, entry, queries, reach, value, sort_queries, outputs, k=None, inputs=None):
        """The one path of the four searches, ``cer_<entry>_f32``: the reach (``method``'s argument ``reach``) rounded to float32 and checked,
        then the queries; ``outputs``: (name, shape of a row, dtype, value on an empty side or None for an output that is not wanted) in the
        entry point's order -> the list of those tensors [m, *row].  ``k`` (checked by the caller) goes in front of the reach, ``inputs(m)`` ->
        (tensor, name) pairs between the reach and the outputs."""
        value = _reach(value, reach)
        queries = _cloud(queries, "queries")
        m, dev = int(queries.shape[0]), queries.device
        inputs = inputs(m) if inputs else ()
        empty = m == 0 or self.n == 0                        # (the entry point launches nothing for an empty side)
        out = [None if fill is None else torch.full((m,) + row, fill, device=dev, dtype=dt) if empty else torch.empty((m,) + row, device=dev, dtype=dt)
               for _, row, dt, fill in outputs]
        if empty:
            return out
        qorder = self._walk_order(queries, m) if sort_queries else None
        rc = getattr(L.load(), f"cer_{entry}_f32")(*self.grid_args(), L.dev_ptr(queries, "queries"), L.dev_ptr(qorder, "qorder", torch.int64), m,
                                                   *(() if k is None else (k,)), value, *[L.dev_ptr(t, name) for t, name in inputs],
                                                   *[L.dev_ptr(t, o[0], o[2]) for t, o in zip(out, outputs)], L.cur_stream())
        if rc == -2:
            raise ValueError(f"{method}: {reach} {value} is more than {GRID_MAX_RINGS} cells of {self.cell}; index the cloud with a larger cell")
        L.check(rc, entry)
        return out

    def nearest(self, queries, max_dist, sort_queries=True):
        """-> (dist float32 [m], idx int64 [m]) in the queries' order: the indexed point with the smallest (d2, index), d2 = (dx*dx + dy*dy) +
        dz*dz in fp64, among those with d2 <= double(max_dist)^2; dist = float32(sqrt(d2)); (inf, -1) where there is none or the query is
        not finite.  ``sort_queries``: walk the queries in the order of their own cells (faster; the result is the same)."""
        idx, dist = self._query("nearest", "grid_nearest", queries, "max_dist", max_dist, sort_queries,
                                (("idx", (), torch.int64, -1), ("dist", (), torch.float32, float("inf"))))
        return dist, idx

    def _knn(self, method, queries, k, max_dist, sort_queries, lists, mean):
        k, inf = _knn_k(k), float("inf")
        idx, dist, count, avg = self._query(method, "grid_knn", queries, "max_dist", max_dist, sort_queries,
                                            (("idx", (k,), torch.int64, -1 if lists else None), ("dist", (k,), torch.float32, inf if lists else None),
                                             ("count", (), torch.int32, 0), ("mean", (), torch.float64, inf if mean else None)), k=k)
        return dist, idx, count, avg

    def knn(self, queries, k, max_dist, sort_queries=True):
        """-> (dist float32 [m, k], idx int64 [m, k], count int32 [m]): per query the min(k, candidates) indexed points with the smallest (d2,
        index), in that order; d2, the candidates (d2 <= double(float32(max_dist))^2) and dist as ``nearest`` defines them.  Unused slots are
        (inf, -1); count = the used ones, 0 for a query that is not finite.  A query that is itself an indexed point finds itself (or a
        duplicate of lower index) first, at 0.  ``k``: 1 .. 32 (KNN_MAX), ValueError otherwise; k = 1 is ``nearest``."""
        dist, idx, count, _ = self._knn("knn", queries, k, max_dist, sort_queries, True, False)
        return dist, idx, count

    def knn_mean_distance(self, queries, k, max_dist, sort_queries=True):
        """-> (mean float64 [m], count int32 [m]): the mean of the fp64 distances sqrt(d2) to the neighbours ``knn`` lists, added in ascending
        order and divided by their number (inf where count = 0) - without the [m, k] lists ever being written."""
        _, _, count, mean = self._knn("knn_mean_distance", queries, k, max_dist, sort_queries, False, True)
        return mean, count

    def count_within(self, queries, radius, sort_queries=True):
        """-> int32 [m]: the number of indexed points with d2 <= double(float32(radius))^2 (``nearest``'s d2; inclusive; the query itself when it
        is an indexed point); 0 for a query that is not finite."""
        return self._query("count_within", "grid_count_within", queries, "radius", radius, sort_queries, (("count", (), torch.int32, 0),))[0]

    def normals(self, queries, k, max_dist, viewpoints=None, sort_queries=True, moments=False):
        """-> (normal float32 [m, 3], curvature float32 [m], count int32 [m]) and, with ``moments``, mom float64 [m, 9]: the plane through the
        neighbours ``knn(queries, k, max_dist)`` lists (count of them; a query that is an indexed point is among its own).  In fp64, about the
        query, in the list's order: S1 = sum d, S2 = sum d_a d_b (xx xy xz yy yz zz) - ``mom`` holds these nine; C = S2 / c - mean mean^T; its
        eigenvalues l0 <= l1 <= l2 by cyclic Jacobi.  A query is VALID iff it is finite, count >= 3, l2 > 0 and l1 > 1e-12 l2 (not collinear):
        normal = the unit eigenvector of l0 rounded once to float32, curvature = max(l0, 0) / (l0 + l1 + l2); otherwise (0, 0, 0) and NaN.
        Sign: the component of largest magnitude is positive (lowest axis on a tie); with ``viewpoints`` (CUDA float32 [3] or [m, 3]) the
        normal is turned so that normal . (viewpoint - query) >= 0; a non-finite viewpoint leaves the canonical sign.  ``k``: 1 .. 32."""
        def inputs(m, viewpoints=viewpoints):
            if viewpoints is not None:
                if not isinstance(viewpoints, torch.Tensor) or not viewpoints.is_cuda:
                    raise RuntimeError("viewpoints must be a CUDA tensor (no CPU fallback)")
                if viewpoints.dtype != torch.float32:
                    raise RuntimeError("viewpoints must be float32")
                if tuple(viewpoints.shape) == (3,):
                    viewpoints = viewpoints.expand(m, 3)
                if tuple(viewpoints.shape) != (m, 3):
                    raise ValueError(f"viewpoints: [3] or one per query [{m}, 3] expected, got {tuple(viewpoints.shape)}")
                viewpoints = viewpoints.contiguous()
            return (self.points, "points"), (viewpoints, "viewpoints")

        out = self._query("normals", "grid_normals", queries, "max_dist", max_dist, sort_queries,
                          (("normal", (3,), torch.float32, 0.0), ("curvature", (), torch.float32, float("nan")), ("count", (), torch.int32, 0),
                           ("mom", (9,), torch.float64, 0.0 if moments else None)), k=_knn_k(k), inputs=inputs)
        return tuple(out) if moments else tuple(out[:3])


def voxel_downsample(points, cell):
    """Indices (int64, ascending) of the lowest-index point of every occupied cell of a grid with edge ``cell`` whose origin is the cloud's
    per-axis minimum: a VOXEL thinning - deterministic, a pure function of the input.  The greedy radius thinning of the DTU MATLAB script
    (which keeps a point unless an earlier kept point lies within the radius) is ``radius_thin``; this one guarantees neither of its two
    properties: kept points of neighbouring cells may be closer than ``cell``, and no two kept points share a cell.  Points with a
    non-finite coordinate are dropped."""
    index = CloudIndex(points, cell)
    return torch.sort(index.heads()).values


def _visit_order(order, seed, n, dev):
    """the visiting order as an int64 tensor on ``dev`` (None: the points' own order)"""
    if isinstance(order, str):
        if order == "index":
            return None
        return torch.randperm(n, generator=torch.Generator("cpu").manual_seed(int(seed))).to(dev)      # made on the host: the same on every machine
    if tuple(order.shape) != (n,):
        raise ValueError(f"order: a permutation of 0 .. {n - 1} expected, got shape {tuple(order.shape)}")
    order = order.to(dev).contiguous()
    if n and not bool((torch.sort(order).values == torch.arange(n, device=dev)).all()):
        raise ValueError(f"order: a permutation of 0 .. {n - 1} expected")
    return order


def radius_thin(points, radius, order="random", seed=0, cell=None, max_rounds=4096, info=None):
    """Indices (int64, ascending) of the points that the greedy radius thinning of the DTU evaluation script (``reducePts_haa``) keeps: visit
    the points in ``order``; a point that is still in the set stays and removes every point within ``radius``.  Exactly: with
    rank[visit[t]] = t, point i is kept iff it is finite and no kept point j with rank[j] < rank[i] has d2(i, j) <= double(float32(radius))^2,
    d2 = (dx*dx + dy*dy) + dz*dz in fp64 on the float32 coordinates (``nearest``'s contract; inclusive, as MATLAB's rangesearch is).  Kept
    points are pairwise farther apart than the radius and every dropped finite point has a kept one within it.  Points with a non-finite
    coordinate are never kept and remove nobody; of exact duplicates the lowest rank survives.  The set is unique: what the sequential loop
    yields for that order, whatever the schedule of the device.

    ``order``: "random" - ``torch.randperm(n, generator=torch.Generator("cpu").manual_seed(seed))``, the script's way; "index" - the points'
    own order; or an int64 tensor, the visiting order itself (a permutation of 0 .. n-1, ValueError otherwise).  ``cell``: the grid's edge,
    default ``radius``.  The device runs rounds until every point is decided; a random order needs around ten, points that are ordered along
    a curve and visited in that order two per kept point: more than ``max_rounds`` raises RuntimeError.  ``info``: a dict that receives
    "rounds", "compactions" (the host reads one number per compaction) and "n_finite"."""
    radius = float(np.float32(radius))
    if not (radius > 0.0 and math.isfinite(radius)):
        raise ValueError("radius must be a positive finite number")
    if isinstance(order, str):
        if order not in ("random", "index"):
            raise ValueError(f'order: "random", "index" or an int64 tensor expected, got {order!r}')
    elif not isinstance(order, torch.Tensor) or order.dtype != torch.int64 or order.dim() != 1:
        raise ValueError('order: "random", "index" or an int64 tensor [n] expected')
    max_rounds = int(max_rounds)
    if max_rounds < 1:
        raise ValueError("max_rounds must be >= 1")
    points = _cloud(points, "points")
    cell = radius if cell is None else _cell(cell)
    if math.ceil(radius / cell) > GRID_MAX_RINGS:
        raise ValueError(f"radius_thin: radius {radius} is more than {GRID_MAX_RINGS} cells of {cell}; use a larger cell")
    n_all, dev = int(points.shape[0]), points.device
    visit = _visit_order(order, seed, n_all, dev)
    stats = {"rounds": 0, "compactions": 0, "n_finite": 0}
    if info is not None:
        info.update(stats)
    if n_all == 0:
        return torch.empty(0, device=dev, dtype=torch.int64)
    # indexed in visiting order: the fourth word of every record is the point's rank, and the state is indexed by rank
    index = CloudIndex(points if visit is None else points.index_select(0, visit), cell)
    stats["n_finite"] = index.n
    if index.n == 0:
        if info is not None:
            info.update(stats)
        return torch.empty(0, device=dev, dtype=torch.int64)
    lib = L.load()
    state = torch.zeros(n_all, device=dev, dtype=torch.uint8)
    partials, offsets, total = L.compaction_buffers(int(lib.cer_grid_partials(index.n)), dev, extra=1, totals=1)
    lists = [torch.empty(index.n, device=dev, dtype=torch.int32) for _ in range(2)]
    grid, pstate = index.grid_args(), L.dev_ptr(state, "state", torch.uint8)
    active, n_active = None, index.n                         # (None: the list 0 .. n-1)
    while n_active:
        if stats["rounds"] >= max_rounds:
            raise RuntimeError(f"radius_thin: {n_active} of {index.n} points are undecided after {max_rounds} rounds - the visiting order follows "
                               'the points along a curve or surface (two rounds per kept point); use order="random", or raise max_rounds')
        pa = L.dev_ptr(active, "active", torch.int32)
        for _ in range(min(THIN_ROUNDS_PER_COMPACTION, max_rounds - stats["rounds"])):
            L.check(lib.cer_grid_thin_round_f32(*grid, pa, n_active, radius, pstate, L.cur_stream()), "grid_thin_round")
            stats["rounds"] += 1
        out = lists[stats["compactions"] & 1]
        L.check(lib.cer_grid_thin_compact_i32(grid[0], index.n, pstate, pa, n_active, L.dev_ptr(partials, "partials", torch.int32),
                                              L.dev_ptr(offsets, "offsets", torch.int64), L.dev_ptr(out, "out", torch.int32),
                                              L.dev_ptr(total, "total", torch.int64), L.cur_stream()), "grid_thin_compact")
        stats["compactions"] += 1
        active, n_active = out, int(total.cpu())             # (the one read per compaction: is anything left)
    if info is not None:
        info.update(stats)
    ranks = torch.nonzero(state == 1).flatten()
    return ranks if visit is None else torch.sort(visit.index_select(0, ranks)).values


# ---------------------------------------------------------------- outlier removal
def _self_search_scale(points, max_dist, cell):
    """-> (the checked cloud, max_dist, cell) of a search of a cloud on itself: ``max_dist`` a finite number >= 0 (rounded to float32), or None
    for 1 % of the diagonal of the bounding box of the finite points (0 without one); ``cell`` a positive finite number, or None for
    ``max_dist / KNN_CELL_DIVISOR``.  ValueError otherwise, before the cloud is looked at."""
    if max_dist is not None:
        max_dist = _reach(max_dist, "max_dist", finite=True)
    cell = None if cell is None else _cell(cell)
    points = _cloud(points, "points")
    n = int(points.shape[0])
    if max_dist is None:
        finite = torch.isfinite(points).all(1, keepdim=True)
        if n and bool(finite.any()):
            lo = torch.where(finite, points, points.new_full((), float("inf"))).amin(0).double()
            hi = torch.where(finite, points, points.new_full((), float("-inf"))).amax(0).double()
            max_dist = float(np.float32(0.01 * float((hi - lo).norm())))
        else:
            max_dist = 0.0
    if cell is None:
        cell = max_dist / KNN_CELL_DIVISOR if max_dist > 0.0 else 1.0        # (a cloud without extent: any cell will do)
    return points, max_dist, cell


def remove_statistical_outliers(points, k=20, std_ratio=2.0, max_dist=None, cell=None, info=None):
    """Indices (int64, ascending) of the points that the statistical outlier filter keeps - Open3D's ``remove_statistical_outlier``, stated
    here in full.  The cloud is indexed on itself, so every point is one of its own ``k`` neighbours (at distance 0).  mean_i =
    ``knn_mean_distance(points, k, max_dist)``; point i is VALID iff it has k neighbours within ``max_dist`` (count_i == k).  mu = the mean of
    the valid mean_i, sigma = sqrt(sum (mean_i - mu)^2 / (n_valid - 1)) over them (fp64 reductions on the device); point i is kept iff it is
    valid and mean_i < mu + std_ratio * sigma.  A point with fewer than k points within ``max_dist``, itself included, is isolated at the scale
    the caller named: it is dropped and enters neither mu nor sigma (nor does a point with a non-finite coordinate).  With fewer than 2 valid
    points every valid point is kept.

    ``max_dist=None``: 1 % of the diagonal of the bounding box of the finite points - distant floaters widen that box, and the scale with it:
    name ``max_dist`` when the cloud's extent is not the surface's.  ``cell=None``: ``max_dist / 4``.  ``info``: a dict that receives "mu",
    "sigma", "threshold", "n_valid", "n_kept", "max_dist" and "cell"."""
    k, std_ratio = _knn_k(k), float(std_ratio)
    if not math.isfinite(std_ratio):
        raise ValueError("std_ratio must be finite")
    points, max_dist, cell = _self_search_scale(points, max_dist, cell)
    n, dev = int(points.shape[0]), points.device
    stats = {"mu": float("nan"), "sigma": float("nan"), "threshold": float("inf"), "n_valid": 0, "n_kept": 0, "max_dist": max_dist, "cell": cell}
    keep = torch.empty(0, device=dev, dtype=torch.int64)
    if n:
        mean, count = CloudIndex(points, cell).knn_mean_distance(points, k, max_dist)
        valid = count == k
        n_valid = int(torch.count_nonzero(valid))
        stats["n_valid"] = n_valid
        if n_valid >= 2:
            zero = torch.zeros_like(mean)
            mu = float(torch.where(valid, mean, zero).sum()) / n_valid
            dev2 = torch.where(valid, mean - mu, zero)
            sigma = math.sqrt(float((dev2 * dev2).sum()) / (n_valid - 1))
            stats.update(mu=mu, sigma=sigma, threshold=mu + std_ratio * sigma)
            valid = valid & (mean < stats["threshold"])
        keep = torch.nonzero(valid).flatten()
    stats["n_kept"] = int(keep.shape[0])
    if info is not None:
        info.update(stats)
    return keep


def remove_radius_outliers(points, radius, min_neighbours, cell=None, info=None):
    """Indices (int64, ascending) of the points with more than ``min_neighbours`` points of the cloud within ``radius`` of them
    (``count_within`` on the cloud itself, so the count includes the point: Open3D's ``remove_radius_outlier``).  Points with a non-finite
    coordinate count nothing and are dropped.  ``cell=None``: ``radius / 4``.  ``info``: a dict that receives "n_kept", "radius" and "cell"."""
    radius = _reach(radius, "radius", finite=True)
    min_neighbours = int(min_neighbours)
    if min_neighbours < 0:
        raise ValueError("min_neighbours must be >= 0")
    if cell is None:
        cell = radius / KNN_CELL_DIVISOR if radius > 0.0 else 1.0
    cell = _cell(cell)
    points = _cloud(points, "points")
    if int(points.shape[0]):
        keep = torch.nonzero(CloudIndex(points, cell).count_within(points, radius) > min_neighbours).flatten()
    else:
        keep = torch.empty(0, device=points.device, dtype=torch.int64)
    if info is not None:
        info.update(n_kept=int(keep.shape[0]), radius=radius, cell=cell)
    return keep


def clean_cloud(points, clean):
    """The filter a ``clean`` dictionary names, on a CUDA float32 cloud -> (kept indices, info): {"method": "statistical", "k", "std_ratio",
    "max_dist"} or {"method": "radius", "radius", "min_neighbours"} (``cell`` is accepted by both; what is left out takes the filter's
    default).  ValueError for another method, a missing ``radius`` / ``min_neighbours`` or a key the filter does not take."""
    if not isinstance(clean, dict) or clean.get("method") not in ("statistical", "radius"):
        raise ValueError('clean: a dict with "method": "statistical" or "radius" expected')
    args = {key: v for key, v in clean.items() if key != "method"}
    allowed = ("k", "std_ratio", "max_dist", "cell") if clean["method"] == "statistical" else ("radius", "min_neighbours", "cell")
    extra = sorted(set(args) - set(allowed))
    if extra:
        raise ValueError(f'clean: method "{clean["method"]}" takes {", ".join(allowed)}; got {", ".join(extra)}')
    info = {"method": clean["method"]}
    if clean["method"] == "statistical":
        return remove_statistical_outliers(points, info=info, **args), info
    if "radius" not in args or "min_neighbours" not in args:
        raise ValueError('clean: method "radius" needs "radius" and "min_neighbours"')
    return remove_radius_outliers(points, info=info, **args), info


# ---------------------------------------------------------------- surface normals
def estimate_normals(points, k=20, max_dist=None, cell=None, viewpoints=None, info=None):
    """-> (normal float32 [n, 3], curvature float32 [n]): ``CloudIndex(points, cell).normals(points, k, max_dist, viewpoints)`` - the cloud
    indexed on itself, so every point is one of its own ``k`` neighbours (Open3D's ``estimate_normals`` with a hybrid kNN / radius search,
    followed by ``orient_normals_towards_camera_location`` when ``viewpoints`` - CUDA float32 [3] or [n, 3] - is given).  A point without a
    plane (fewer than 3 neighbours within ``max_dist``, collinear or coincident ones, a non-finite coordinate) has normal (0, 0, 0) and
    curvature NaN.  ``max_dist`` / ``cell``: as ``remove_statistical_outliers`` (None: 1 % of the bounding-box diagonal / ``max_dist / 4``).
    ``info``: a dict that receives "n_valid" (one host read), "max_dist", "cell" and "k"."""
    k = _knn_k(k)
    points, max_dist, cell = _self_search_scale(points, max_dist, cell)
    normal, curvature, _ = CloudIndex(points, cell).normals(points, k, max_dist, viewpoints=viewpoints)
    if info is not None:
        info.update(n_valid=int(torch.count_nonzero(~torch.isnan(curvature))), max_dist=max_dist, cell=cell, k=k)
    return normal, curvature


def normals_options(normals):
    """The arguments of ``estimate_normals`` that ``reconstruct_scan(normals=...)`` names: True -> {}; a dict with any of "k", "max_dist", "cell"
    -> a copy; ValueError for anything else or a key beyond those."""
    if normals is True:
        return {}
    if not isinstance(normals, dict):
        raise ValueError('normals: None, True or a dict with "k", "max_dist", "cell" expected')
    allowed = ("k", "max_dist", "cell")
    extra = sorted(set(normals) - set(allowed))
    if extra:
        raise ValueError(f'normals: takes {", ".join(allowed)}; got {", ".join(str(e) for e in extra)}')
    return dict(normals)


def cloud_distances(src, dst, max_dist, cell=None):
    """float32 [len(src)]: the distance from every ``src`` point to its nearest ``dst`` point within ``max_dist`` (inf where there is none).
    ``cell`` defaults to ``max_dist / 4`` (DEFAULT_CELL_DIVISOR: measured)."""
    cell = float(max_dist) / DEFAULT_CELL_DIVISOR if cell is None else cell
    return CloudIndex(dst, cell).nearest(src, max_dist)[0]


def _is_tensor(d):
    return isinstance(d, torch.Tensor)


def _f64(d):
    return d.double() if _is_tensor(d) else np.asarray(d).astype(np.float64)


def _count(mask):
    return int(torch.count_nonzero(mask)) if _is_tensor(mask) else int(np.count_nonzero(mask))


def _mean_below(d, bound):
    """(mean of the entries < bound - nan if there are none, their count); d is fp64, so the comparison is with ``bound`` itself, not with
    its float32 rounding"""
    inside = d < bound
    k = _count(inside)
    s = float((torch.where(inside, d, torch.zeros_like(d)) if _is_tensor(d) else np.where(inside, d, 0.0)).sum())
    return (s / k if k else float("nan")), k


def metrics_from_distances(d_pred, d_gt, max_dist, tau=None):
    """The arithmetic of both protocols on two distance vectors (numpy arrays or tensors; d_pred: predicted -> ground truth, d_gt: the other
    way).  accuracy = mean of d_pred over d_pred < max_dist, completeness = the same of d_gt, overall = their mean (nan where a mean has no
    entries); with ``tau``: precision = share of d_pred < tau, recall = share of d_gt < tau (0 for an empty vector), fscore = their harmonic
    mean, 0 when both are 0.  The distances are promoted to fp64 first: comparisons, sums and counts are fp64."""
    d_pred, d_gt = _f64(d_pred), _f64(d_gt)
    acc, n_pred_in = _mean_below(d_pred, max_dist)
    comp, n_gt_in = _mean_below(d_gt, max_dist)
    out = {"accuracy": acc, "completeness": comp, "overall": 0.5 * (acc + comp), "n_pred": int(len(d_pred)), "n_gt": int(len(d_gt)),
           "n_pred_in": n_pred_in, "n_gt_in": n_gt_in}
    if tau is not None:
        p = _count(d_pred < tau) / len(d_pred) if len(d_pred) else 0.0
        r = _count(d_gt < tau) / len(d_gt) if len(d_gt) else 0.0
        out.update(precision=p, recall=r, fscore=2.0 * p * r / (p + r) if p + r > 0.0 else 0.0, tau=float(tau))
    return out


def _keep(points, keep, name):
    if keep is None:
        return None
    keep = torch.as_tensor(keep, device=points.device)
    if keep.dtype != torch.bool or tuple(keep.shape) != (points.shape[0],):
        raise ValueError(f"{name}: a boolean mask with one entry per point expected")
    return keep


def _thin(pred, thin, thin_method, thin_seed):
    return radius_thin(pred, thin, seed=thin_seed) if thin_method == "greedy" else voxel_downsample(pred, thin)


def accuracy_completeness(pred, gt, max_dist=20.0, thin=None, keep_pred=None, keep_gt=None, cell=None, thin_method="voxel", thin_seed=0,
                          align=None):
    """The DTU protocol.  ``pred`` is first thinned if ``thin`` is given: with ``voxel_downsample(pred, thin)`` (``thin_method="voxel"``, the
    default: one point per cell of that edge) or with ``radius_thin(pred, thin, seed=thin_seed)`` (``"greedy"``: the MATLAB script's own
    reduction, visiting the points in a seeded random order).  accuracy = mean distance pred -> gt over the points with d < max_dist, completeness = the same gt -> pred, overall =
    their mean.  ``keep_pred`` / ``keep_gt``: optional boolean masks (one entry per point of ``pred`` as passed in / of ``gt``) selecting
    which points enter the two means - where a caller applies DTU's observability mask and ground plane; every point still serves as a
    neighbour.  -> {"accuracy", "completeness", "overall", "n_pred", "n_gt", "n_pred_in", "n_gt_in"}: n_pred / n_gt are the points that were
    measured (after thinning and masks), n_*_in those within max_dist.  ``align``: a 4x4 rigid motion applied to ``pred`` with
    ``rigid_transform`` before anything else (``icp`` / ``register`` find one)."""
    if thin_method not in ("voxel", "greedy"):
        raise ValueError(f'thin_method: "voxel" or "greedy" expected, got {thin_method!r}')
    if align is not None:
        pred = rigid_transform(pred, align)
    pred, gt = _cloud(pred, "pred"), _cloud(gt, "gt")
    kp, kg = _keep(pred, keep_pred, "keep_pred"), _keep(gt, keep_gt, "keep_gt")
    if thin is not None:
        sel = _thin(pred, thin, thin_method, thin_seed)
        pred = pred.index_select(0, sel)
        kp = kp.index_select(0, sel) if kp is not None else None
    cell = float(max_dist) / DEFAULT_CELL_DIVISOR if cell is None else cell
    d_pred = CloudIndex(gt, cell).nearest(pred, max_dist)[0]
    d_gt = CloudIndex(pred, cell).nearest(gt, max_dist)[0]
    if kp is not None:
        d_pred = d_pred[kp]
    if kg is not None:
        d_gt = d_gt[kg]
    return metrics_from_distances(d_pred, d_gt, max_dist)


def fscore(pred, gt, tau, cell=None, align=None):
    """The Tanks-and-Temples protocol: precision = share of ``pred`` within ``tau`` of ``gt`` (d < tau), recall = share of ``gt`` within ``tau``
    of ``pred``, fscore = their harmonic mean (0 when both are 0).  -> {"precision", "recall", "fscore", "tau", "n_pred", "n_gt"}.
    ``align``: a 4x4 rigid motion applied to ``pred`` with ``rigid_transform`` before anything else."""
    if align is not None:
        pred = rigid_transform(pred, align)
    pred, gt = _cloud(pred, "pred"), _cloud(gt, "gt")
    tau32 = float(np.float32(tau))
    cut = float(np.nextafter(np.float32(tau32), np.float32(np.inf))) if tau32 < float(tau) else tau32      # a float32 cut-off that is not below tau
    d_pred = cloud_distances(pred, gt, cut, cell)
    d_gt = cloud_distances(gt, pred, cut, cell)
    m = metrics_from_distances(d_pred, d_gt, cut, tau=tau)
    return {k: m[k] for k in ("precision", "recall", "fscore", "tau", "n_pred", "n_gt")}


# ---------------------------------------------------------------- rigid registration (csrc/cloud_align.hip)
def _rigid(T, name="T"):
    """-> 4x4 float64 numpy; ValueError unless ``T`` is a finite 4x4 whose last row is 0 0 0 1"""
    if isinstance(T, torch.Tensor):
        T = T.detach().double().cpu().numpy()
    try:
        T = np.array(T, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{name}: a 4x4 matrix expected") from e
    if T.shape != (4, 4):
        raise ValueError(f"{name}: a 4x4 matrix expected, got shape {T.shape}")
    if not np.isfinite(T).all():
        raise ValueError(f"{name}: finite entries expected")
    if not np.array_equal(T[3], (0.0, 0.0, 0.0, 1.0)):
        raise ValueError(f"{name}: the last row of a rigid motion is 0 0 0 1, got {T[3].tolist()}")
    return T


def _transform(points, T):                                   # points: a checked cloud, T: a checked 4x4
    n = int(points.shape[0])
    out = torch.empty(n, 3, device=points.device, dtype=torch.float32)
    rows = (ctypes.c_double * 12)(*[float(v) for v in T[:3].reshape(-1)])
    L.check(L.load().cer_cloud_transform_f32(L.dev_ptr(points, "points"), n, rows, L.dev_ptr(out, "out"), L.cur_stream()), "cloud_transform")
    return out


def rigid_transform(points, T):
    """A new float32 [n, 3]: ``T`` (4x4, numpy or tensor, taken as fp64; last row 0 0 0 1, ValueError otherwise) applied to every point:
    out[i][r] = float32(((T[r][0] * x + T[r][1] * y) + T[r][2] * z) + T[r][3]) with x, y, z promoted to fp64 - that association, no fused
    multiply-add, one rounding to float32.  Non-finite coordinates propagate by IEEE rules."""
    T = _rigid(T)
    return _transform(_cloud(points, "points"), T)


def _pivot(pivot):
    pivot = np.zeros(3) if pivot is None else np.array(pivot, dtype=np.float64).reshape(-1)
    if pivot.shape != (3,) or not np.isfinite(pivot).all():
        raise ValueError("pivot: three finite numbers expected")
    return pivot


def _moments(a, b, idx, pivot):                              # checked clouds, idx int64 [len(a)] on their device, pivot: 3 doubles
    m, dev = int(a.shape[0]), a.device
    if m == 0:
        return np.zeros(MOMENT_COUNT)
    lib = L.load()
    partials = torch.empty(MOMENT_COUNT * int(lib.cer_cloud_moment_partials(m)), device=dev, dtype=torch.float64)
    out = torch.empty(MOMENT_COUNT, device=dev, dtype=torch.float64)
    L.check(lib.cer_cloud_pair_moments_f64(L.dev_ptr(a, "a"), L.dev_ptr(b, "b"), L.dev_ptr(idx, "idx", torch.int64), m,
                                           (ctypes.c_double * 3)(*[float(v) for v in pivot]), L.dev_ptr(partials, "partials", torch.float64),
                                           L.dev_ptr(out, "out", torch.float64), L.cur_stream()), "cloud_pair_moments")
    return out.cpu().numpy()


def pair_moments(a, b, idx, pivot=None):
    """numpy float64 [17]: the sums over the pairs (a[i], b[idx[i]]), i with idx[i] >= 0 (``nearest``'s -1: no pair) and a finite a[i].  With
    A = double(a) - pivot and B = double(b) - pivot (``pivot``: three numbers, default 0 0 0; near the clouds it keeps the covariance free of
    cancellation): [0] k, the number of pairs; [1:4] sum A; [4:7] sum B; [7:16] sum of the outer product A x B (row: A's axis); [16] sum of
    |a - b|^2 as ``nearest`` forms d2.  fp64, a fixed summation tree: the same bits on every run.  Returning them is the one
    host read.  ``idx``: int64 [len(a)], every entry -1 or a row of ``b`` (ValueError otherwise)."""
    pivot = _pivot(pivot)
    a, b = _cloud(a, "a"), _cloud(b, "b")
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or tuple(idx.shape) != (a.shape[0],):
        raise ValueError("idx: an int64 tensor with one entry per point of a expected")
    idx = idx.to(a.device).contiguous()
    if len(idx) and (int(idx.max()) >= int(b.shape[0]) or int(idx.min()) < -1):
        raise ValueError(f"idx: entries in -1 .. {int(b.shape[0]) - 1} expected")
    return _moments(a, b, idx, pivot)


def rigid_from_moments(mom, pivot=(0.0, 0.0, 0.0)):
    """The least-squares rigid motion of the pairs behind ``mom`` (``pair_moments`` taken about ``pivot``) as a 4x4 float64 - Kabsch: with the
    means Abar, Bbar and H = sum A x B - k Abar x Bbar = U S V^T, R = V diag(1, 1, det(V U^T)) U^T and t = (Bbar + pivot) - R (Abar + pivot).
    Pure numpy.  ValueError for fewer than 3 pairs and for collinear pairs (second singular value <= 1e-12 of the first: the rotation about
    their line is not determined); planar pairs are fine, the det term picks the proper rotation."""
    mom = np.array(mom, dtype=np.float64).reshape(-1)
    if mom.shape != (MOMENT_COUNT,):
        raise ValueError(f"mom: {MOMENT_COUNT} sums expected")
    pivot = _pivot(pivot)
    k = mom[0]
    if not k >= 3:
        raise ValueError(f"rigid_from_moments: at least 3 pairs expected, got {k:g}")
    abar, bbar = mom[1:4] / k, mom[4:7] / k
    H = mom[7:16].reshape(3, 3) - k * np.outer(abar, bbar)
    U, S, Vt = np.linalg.svd(H)
    if not S[1] > COLLINEAR_RATIO * S[0]:
        raise ValueError("rigid_from_moments: the pairs are collinear (or coincide); the rotation is not determined")
    V = Vt.T
    R = V @ np.diag((1.0, 1.0, float(np.sign(np.linalg.det(V @ U.T))))) @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (bbar + pivot) - R @ (abar + pivot)
    return T


# ---------------------------------------------------------------- point-to-plane
def _normals_of(normals, cloud, name):
    """``normals`` as a contiguous float32 [len(cloud), 3] on ``cloud``'s device, or the error that says what it is not"""
    if not isinstance(normals, torch.Tensor) or not normals.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor (no CPU fallback)")
    if normals.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32")
    if tuple(normals.shape) != (int(cloud.shape[0]), 3) or normals.device != cloud.device:
        raise ValueError(f"{name}: float32 [{int(cloud.shape[0])}, 3] on the cloud's device expected, got {tuple(normals.shape)} on {normals.device}")
    return normals.contiguous()


def _plane_moments(a, b, nrm, idx, pivot):                   # checked clouds and normals, idx int64 [len(a)] on their device, pivot: 3 doubles
    m, dev = int(a.shape[0]), a.device
    if m == 0:
        return np.zeros(PLANE_MOMENT_COUNT)
    lib = L.load()
    partials = torch.empty(PLANE_MOMENT_COUNT * int(lib.cer_cloud_plane_moment_partials(m)), device=dev, dtype=torch.float64)
    out = torch.empty(PLANE_MOMENT_COUNT, device=dev, dtype=torch.float64)
    L.check(lib.cer_cloud_plane_moments_f64(L.dev_ptr(a, "a"), L.dev_ptr(b, "b"), L.dev_ptr(nrm, "normals"), L.dev_ptr(idx, "idx", torch.int64), m,
                                            (ctypes.c_double * 3)(*[float(v) for v in pivot]), L.dev_ptr(partials, "partials", torch.float64),
                                            L.dev_ptr(out, "out", torch.float64), L.cur_stream()), "cloud_plane_moments")
    return out.cpu().numpy()


def plane_moments(a, b, normals, idx, pivot=None):
    """numpy float64 [30]: the normal equations of one point-to-plane step over the pairs (a[i], b[q], n = normals[q]), q = idx[i] >= 0, a[i]
    finite, n finite and not (0, 0, 0) (``estimate_normals``' "no plane": such a match makes no pair).  ``normals``: float32 [len(b), 3] on
    the clouds' device, used as given, not normalised.  With A = double(a) - pivot, D = double(a) - double(b), r = (Dx*nx + Dy*ny) + Dz*nz
    (the plane residual), c = A x n and J = (c0, c1, c2, n0, n1, n2): [0] k, the number of pairs; [1:22] the upper triangle of sum J_i J_j,
    row-major; [22:28] sum J_i r; [28] sum r^2; [29] sum |a - b|^2 as ``nearest`` forms d2.  fp64, no fused multiply-add, ``pair_moments``'
    summation tree: the same bits on every run.  Returning them is the one host read.  ``idx`` as ``pair_moments`` takes it."""
    pivot = _pivot(pivot)
    a, b = _cloud(a, "a"), _cloud(b, "b")
    normals = _normals_of(normals, b, "normals")
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or tuple(idx.shape) != (a.shape[0],):
        raise ValueError("idx: an int64 tensor with one entry per point of a expected")
    idx = idx.to(a.device).contiguous()
    if len(idx) and (int(idx.max()) >= int(b.shape[0]) or int(idx.min()) < -1):
        raise ValueError(f"idx: entries in -1 .. {int(b.shape[0]) - 1} expected")
    return _plane_moments(a, b, normals, idx, pivot)


def rigid_from_plane_moments(mom, pivot=(0.0, 0.0, 0.0)):
    """The point-to-plane step of the pairs behind ``mom`` (``plane_moments`` taken about ``pivot``) as a 4x4 float64: x = (w, t) minimises
    sum (r + J x)^2, the residual after a small rotation w about the pivot and a translation t - M x = -g with M the symmetric 6x6 of
    [1:22] and g = [22:28].  Solved with the diagonal scaled to 1 (s_i = 1 / sqrt(M_ii), Ms = s s^T * M, x = s * solve(Ms, -(s * g))), which
    makes the degeneracy test independent of the units and of the pivot's distance.  The step is p -> pivot + R (p - pivot) + t with R =
    exp([w]x) by Rodrigues' formula (the series I + K + K^2 / 2 below |w| = 1e-8): an exact rotation of the linearised solution, not the
    Euler-angle composition Open3D's TransformationEstimationPointToPlane builds from the same x.  Pure numpy.  ValueError for fewer than 6
    pairs, for an M_ii <= 0 (a degree of freedom nothing constrains) and for a smallest eigenvalue of Ms <= 1e-10: a plane, a sphere with
    radial normals, a cylinder - some motion slides the target on itself and the step is not determined."""
    mom = np.array(mom, dtype=np.float64).reshape(-1)
    if mom.shape != (PLANE_MOMENT_COUNT,):
        raise ValueError(f"mom: {PLANE_MOMENT_COUNT} sums expected")
    pivot = _pivot(pivot)
    if not mom[0] >= 6:
        raise ValueError(f"rigid_from_plane_moments: at least 6 pairs expected, got {mom[0]:g}")
    M = np.zeros((6, 6))
    M[np.triu_indices(6)] = mom[1:22]
    M = M + np.triu(M, 1).T
    g = mom[22:28].copy()
    diag = np.diag(M)
    if not (diag > 0.0).all():
        raise ValueError("rigid_from_plane_moments: a diagonal entry of the normal matrix is not positive; the pairs do not constrain the motion")
    s = 1.0 / np.sqrt(diag)
    Ms = np.outer(s, s) * M
    if not np.linalg.eigvalsh(Ms)[0] > PLANE_DEGENERATE:
        raise ValueError("rigid_from_plane_moments: the pairs are degenerate (a plane, a sphere, a cylinder: some motion slides the target on "
                         "itself); the step is not determined")
    x = s * np.linalg.solve(Ms, -(s * g))
    w = x[:3]
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    th = math.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    if th < 1e-8:
        R = np.eye(3) + K + 0.5 * (K @ K)
    else:
        R = np.eye(3) + (math.sin(th) / th) * K + ((1.0 - math.cos(th)) / (th * th)) * (K @ K)
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (pivot - R @ pivot) + x[3:]
    return T


def _is_plane(method, dst_normals, normals):
    """``method`` and what may go with it, checked before anything else is looked at -> True for "plane" """
    if method not in ("point", "plane"):
        raise ValueError(f'method: "point" or "plane" expected, got {method!r}')
    if method == "point" and (dst_normals is not None or normals is not None):
        raise ValueError('dst_normals / normals go with method="plane"; method="point" uses no normals')
    return method == "plane"


def _target_normals(plane, dst, dst_normals, normals):
    """None unless ``plane``; else the normals of the checked cloud ``dst``: ``dst_normals``, or estimated (once) with ``normals``' options"""
    if not plane:
        return None
    if dst_normals is not None:
        if normals is not None:
            raise ValueError("normals: options of the estimation; dst_normals were given, nothing is estimated")
        return _normals_of(dst_normals, dst, "dst_normals")
    options = normals_options(normals or True)
    return estimate_normals(dst, **options)[0] if int(dst.shape[0]) else dst.new_zeros(0, 3)


def _icp_args(max_dist, init, max_iter, tol_fitness, tol_rmse):
    max_dist = float(np.float32(max_dist))
    if not (max_dist > 0.0 and math.isfinite(max_dist)):
        raise ValueError("max_dist must be a positive finite number")
    max_iter = int(max_iter)
    if max_iter < 1:
        raise ValueError("max_iter must be >= 1")
    tol_fitness, tol_rmse = float(tol_fitness), float(tol_rmse)
    if not (tol_fitness >= 0.0 and tol_rmse >= 0.0):
        raise ValueError("tol_fitness and tol_rmse must be >= 0")
    return max_dist, (np.eye(4) if init is None else _rigid(init, "init")), max_iter, tol_fitness, tol_rmse


def icp(src, dst, max_dist, init=None, max_iter=50, tol_fitness=1e-6, tol_rmse=1e-6, cell=None, index=None, method="point", dst_normals=None,
        normals=None):
    """ICP of ``src`` onto ``dst`` (CUDA float32 [n, 3] each), from ``init`` (4x4, default the identity); point-to-point unless
    ``method="plane"`` (below).  ``dst`` is indexed
    once (``CloudIndex(dst, cell)``, ``cell`` default ``max_dist / 4``; or the caller's ``index``, which must be over ``dst``).  An iteration:
    cur = rigid_transform(src, T) - always from the original ``src`` with the accumulated fp64 T: one rounding, no drift; index.nearest(cur,
    max_dist); the moments of the pairs about the index's origin; fitness = pairs / len(src), rmse = sqrt(mean d2 of the pairs); stop when
    both moved by less than their tolerance since the iteration before (Open3D's criterion, which the Tanks-and-Temples script uses), else
    T <- rigid_from_moments(...) @ T on the host.  One host read per iteration, at most ``max_iter`` iterations.

    -> {"T": 4x4 float64 numpy, src -> dst's frame; "iterations": evaluations made; "converged"; "fitness", "rmse", "n_pairs": of the last
    evaluation (when ``max_iter`` ends the loop: the one before the last update of T); "history": [(fitness, rmse), ...]}.  Fewer than 3
    pairs (empty clouds included) stop the loop with converged = False and T as it stands; collinear pairs raise ValueError.

    ``method="plane"``: point-to-plane ICP (Chen & Medioni; Open3D's TransformationEstimationPointToPlane) - the same loop with
    ``plane_moments`` about the index's origin and ``rigid_from_plane_moments`` as the step.  A match whose target normal is (0, 0, 0) or
    not finite makes no pair; fitness = pairs / len(src); rmse = sqrt(mean r^2), the PLANE residual (Open3D's definition for this
    estimator); the dict gains "rmse_point" = sqrt(mean d2 of the pairs) and every history entry carries it as a third element.  The loop
    stops below 6 pairs; a degenerate target (a plane, a sphere, a cylinder) raises ValueError.  ``dst_normals``: float32 [len(dst), 3] on
    the device, used as given; None: ``estimate_normals(dst, **normals_options(normals or True))``, once (``normals``: a dict with any of
    "k", "max_dist", "cell").  Either of them with ``method="point"`` is a ValueError, as is any other method."""
    plane = _is_plane(method, dst_normals, normals)
    max_dist, T, max_iter, tol_fitness, tol_rmse = _icp_args(max_dist, init, max_iter, tol_fitness, tol_rmse)
    src, dst = _cloud(src, "src"), _cloud(dst, "dst")
    nrm = _target_normals(plane, dst, dst_normals, normals)
    if index is None:
        index = CloudIndex(dst, float(max_dist) / DEFAULT_CELL_DIVISOR if cell is None else cell)
    elif not isinstance(index, CloudIndex) or index.points.shape != dst.shape or index.points.device != dst.device:
        raise ValueError("index: a CloudIndex over dst expected")
    n = int(src.shape[0])
    out = {"T": T, "iterations": 0, "converged": False, "fitness": 0.0, "rmse": 0.0, "n_pairs": 0, "history": []}
    if plane:
        out["rmse_point"] = 0.0
    if n == 0 or index.n == 0:
        return out
    pivot = np.array([float(v) for v in index.origin])
    for _ in range(max_iter):
        cur = _transform(src, T)
        idx = index.nearest(cur, max_dist)[1]
        mom = _plane_moments(cur, index.points, nrm, idx, pivot) if plane else _moments(cur, index.points, idx, pivot)      # (the one host read)
        k = int(mom[0])
        fitness, rmse = k / n, (math.sqrt(mom[28 if plane else 16] / k) if k else 0.0)
        moved = (abs(fitness - out["fitness"]), abs(rmse - out["rmse"])) if out["iterations"] else None
        out.update(iterations=out["iterations"] + 1, fitness=fitness, rmse=rmse, n_pairs=k)
        if plane:
            out["rmse_point"] = math.sqrt(mom[29] / k) if k else 0.0
            out["history"].append((fitness, rmse, out["rmse_point"]))
        else:
            out["history"].append((fitness, rmse))
        if k < (6 if plane else 3):
            break
        if moved is not None and moved[0] < tol_fitness and moved[1] < tol_rmse:
            out["converged"] = True
            break
        T = (rigid_from_plane_moments(mom, pivot) if plane else rigid_from_moments(mom, pivot)) @ T
        out["T"] = T
    return out


def register(src, dst, stages, init=None, method="point", dst_normals=None, normals=None):
    """Coarse-to-fine ICP: ``stages`` is a sequence of (voxel, max_dist, max_iter); every stage runs ``icp`` on ``voxel_downsample`` of both
    clouds with that edge (voxel None: the clouds as they are) from the stage before's T (the first from ``init``).  -> the last stage's dict
    plus "stages", the list of every stage's dict.  ``method`` / ``dst_normals`` / ``normals``: as ``icp`` takes them; with ``"plane"`` the
    normals are those of the FULL ``dst`` (given, or estimated once - not per stage: a thinned cloud has another surface scale), and a
    stage's voxel selection of ``dst`` selects their rows with it."""
    plane = _is_plane(method, dst_normals, normals)
    try:
        stages = [(None if v is None else _cell(v), float(d), int(it)) for v, d, it in stages]
    except (TypeError, ValueError) as e:
        raise ValueError("stages: a sequence of (voxel or None, max_dist, max_iter) expected") from e
    if not stages:
        raise ValueError("stages: at least one stage expected")
    for _, d, it in stages:
        _icp_args(d, None, it, 0.0, 0.0)
    T = np.eye(4) if init is None else _rigid(init, "init")
    src, dst = _cloud(src, "src"), _cloud(dst, "dst")
    nrm = _target_normals(plane, dst, dst_normals, normals)
    done = []
    for voxel, max_dist, max_iter in stages:
        s = src if voxel is None else src.index_select(0, voxel_downsample(src, voxel))
        sel = None if voxel is None else voxel_downsample(dst, voxel)
        d, n = (dst, nrm) if sel is None else (dst.index_select(0, sel), nrm.index_select(0, sel) if plane else None)
        done.append(icp(s, d, max_dist, init=T, max_iter=max_iter, **({"method": "plane", "dst_normals": n} if plane else {})))
        T = done[-1]["T"]
    return {**done[-1], "stages": done}


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2",
              "int": "<i4", "int32": "<i4", "uint": "<u4", "uint32": "<u4", "float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8"}


def read_ply(path, normals=False):
    """-> (xyz float32 [n, 3], rgb uint8 [n, 3] or None): the vertex element of a binary little-endian PLY whose vertex properties are scalars
    in any order (what ``fusion.write_ply`` writes; extra properties are skipped).  x, y, z must be float, red / green / blue (if all three
    are there) uchar.  ASCII and big-endian files raise ValueError naming the format.  ``normals=True``: a third value, float32 [n, 3] from
    the float properties nx, ny, nz, or None when the file does not have all three."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = raw[:end].decode("ascii").split("\n")
    fmt = next((ln.split()[1] for ln in lines if ln.startswith("format ")), None)
    if fmt != "binary_little_endian":
        raise ValueError(f"{path}: PLY format {fmt!r} is not supported, only binary_little_endian")
    n, fields, element, offset = 0, [], None, 0
    for ln in lines:
        tok = ln.split()
        if not tok:
            continue
        if tok[0] == "element":
            if element == "vertex":
                break                                        # the vertex element is read only if it comes first (it does in every MVS cloud)
            element = tok[1]
            if element != "vertex":
                raise ValueError(f"{path}: element {element!r} in front of the vertices is not supported")
            n = int(tok[2])
        elif tok[0] == "property" and element == "vertex":
            if tok[1] == "list" or tok[1] not in _PLY_TYPES:
                raise ValueError(f"{path}: vertex property {ln!r} is not supported")
            fields.append((tok[2], _PLY_TYPES[tok[1]]))
    names = [k for k, _ in fields]
    if len(set(names)) != len(names) or not all(k in names for k in "xyz"):
        raise ValueError(f"{path}: vertex properties x, y, z expected once each")
    dt = np.dtype(fields)
    body = raw[end + len(b"end_header\n"):]
    if len(body) < n * dt.itemsize:
        raise ValueError(f"{path}: {n} vertices of {dt.itemsize} bytes expected, {len(body)} bytes found")
    v = np.frombuffer(body, dtype=dt, count=n, offset=offset)
    if any(dt[k] != np.dtype("<f4") for k in "xyz"):
        raise ValueError(f"{path}: float x, y, z expected")
    xyz = np.stack([v["x"], v["y"], v["z"]], 1) if n else np.zeros((0, 3), np.float32)
    rgb = None
    if all(k in names for k in ("red", "green", "blue")):
        if any(dt[k] != np.dtype("u1") for k in ("red", "green", "blue")):
            raise ValueError(f"{path}: uchar red, green, blue expected")
        rgb = np.stack([v["red"], v["green"], v["blue"]], 1) if n else np.zeros((0, 3), np.uint8)
    xyz = np.ascontiguousarray(xyz, dtype=np.float32)
    if not normals:
        return xyz, rgb
    nrm = None
    if all(k in names for k in ("nx", "ny", "nz")):
        if any(dt[k] != np.dtype("<f4") for k in ("nx", "ny", "nz")):
            raise ValueError(f"{path}: float nx, ny, nz expected")
        nrm = np.ascontiguousarray(np.stack([v["nx"], v["ny"], v["nz"]], 1) if n else np.zeros((0, 3), np.float32), dtype=np.float32)
    return xyz, rgb, nrm
