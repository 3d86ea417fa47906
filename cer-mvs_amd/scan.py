"""Scan session: every image of a scan is uploaded, prepared and encoded by ``fnet`` ONCE; each depth map then costs ``cnet`` on its
reference view, the cost volumes and the GRU loop.

``inference()`` mirrors the reference driver's loop (inference.py:37-66): one independent stack per reference view.  A scan of M images
with ten neighbours per view makes that loop resize (on the CPU), upload and ``fnet``-encode every image about eleven times.  None of
the three depends on the stack: the resize and the crop are the same for the whole scan, instance norm is per image (a batched
``fnet`` launch equals per-image launches bit for bit, tests/test_hip_parity.py), and ``scale`` multiplies the poses, not the images.

``ScanSession`` keeps, on the device, the prepared images [M,3,H,W] (``cnet`` needs the reference view; the fallback needs stacks) and
one block of split-f16 feature planes per image, in the bordered source-view layout that ``HipEncoder.features_split`` writes and
``ops.cost_build(split=(f1s, store, slots))`` reads through a slot table.  The reference view's plain map is copied out of its block
(``ops.feat_ref_rows``: the 1x1 feature head computes a texel from that texel alone, so the interior of the bordered form holds the plain
form's bits), which keeps one layout per image instead of two.  ``RAFT.forward_cached`` runs the stages on them: the same code on the
same bits as ``RAFT.forward`` on the stack of those images, so the same disparity.

Where the cached path cannot apply - whenever the model's forward would not take its direct-split path (``RAFT.supports_cached``: "LR"
encoders, ``precision="amp"``, MIOpen encoders, a view_group, a stage with D > 64, the fp32 cost-volume walk, overflow_policy
"fallback") - the session hands stacks gathered from the prepared images to the ordinary forward (``cached == False``): the single
upload and the device-side preparation still apply.

The drivers are short callers of pipeline.py and inference.py: ``submit`` is the pipeline's ``pick`` and ``launch`` around the choice between store and
stack, ``depths`` and ``inference_scan`` run ``pipeline.checked`` (the latter through ``inference.run_jobs``, which writes the files), and
``reconstruct_scan`` reads as its steps: ``_depth_stacks``, ``_merged`` and the vote loop, ``_cloud_tail``, then the files."""
import time
from pathlib import Path

import numpy as np
import torch

from . import fusion as FU
from . import ops
from .inference import depth_file, run_jobs, write_pfm
from .pipeline import DepthMapPipeline, calibrating, checked, running_model, stream_count, unwrap


def scan_intrinsics(intrinsics, H0, W0, rescale=1, crop=None):
    """[M,3,3] intrinsics of H0 x W0 images -> those of the prepared images: rows 0 and 1 times ``rescale``, then the principal point
    shifted by the crop window's origin - the arithmetic of inference.scale_operation + crop_operation, operation for operation.  Out of
    place, CPU or device."""
    _, _, y0, x0, _, _ = ops.prep_geometry(H0, W0, rescale, crop)
    intrinsics = intrinsics.clone()
    intrinsics[:, 0] *= rescale
    intrinsics[:, 1] *= rescale
    if crop is not None:
        intrinsics = intrinsics.clone()
        intrinsics[:, 0, 2] -= x0
        intrinsics[:, 1, 2] -= y0
    return intrinsics


def _image_hw(img):
    if img.dim() != 3:
        raise ValueError("ScanSession: every image is uint8 [H,W,3] or float [3,H,W]")
    if img.dtype == torch.uint8:
        return int(img.shape[0]), int(img.shape[1])
    return int(img.shape[1]), int(img.shape[2])


class ScanSession:
    """``images``: list or tensor of M images, uint8 [H0,W0,3] (``bgr``: as OpenCV reads them) or float [3,H0,W0] with values 0..255, host
    or device, all of one size.  ``poses`` [M,4,4]; ``intrinsics`` [M,3,3], unscaled.  ``model``: a test-mode RAFT on the GPU.

    ``depth(ref, srcs, scale)`` -> what ``model(stack, poses[idx], intrinsics'[idx], scale=scale)`` returns for idx = [ref] + srcs, the stack
    gathered from ``self.prepared`` and intrinsics' = ``self.intrinsics``.  ``submit`` / ``result`` keep ``streams`` depth maps in flight
    (one replica of the model per stream, pipeline.DepthMapPipeline's; the store and the prepared images are shared and read-only)."""

    @staticmethod
    def bytes_needed(M, H, W):
        """Device bytes a session keeps for a scan of M prepared images of H x W: the fp32 images and, per image, one bordered block of
        split-f16 feature planes ((H/4 + 4) * (W/4 + 4) texels x 128 halves).  The model's replicas and the workspaces of the forwards
        in flight come on top."""
        h, w = H // 4, W // 4
        return M * 3 * H * W * 4 + M * (h + 4) * (w + 4) * 128 * 2

    def __init__(self, model, images, poses, intrinsics, rescale=1, crop=None, streams=3, encode_batch=4, max_bytes=None, bgr=False,
                 force_uncached=False):
        core = unwrap(model)
        if not core.test_mode:
            raise RuntimeError("ScanSession: the model must be built with test_mode=True")
        dev = next(core.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("ScanSession: the model must live on a GPU (there is no CPU path)")
        core.eval()
        self.model, self.device = core, dev
        images = list(images) if not isinstance(images, torch.Tensor) else [images[i] for i in range(images.shape[0])]
        images = [torch.as_tensor(im) for im in images]
        M = len(images)
        if M < 2:
            raise ValueError("ScanSession: a scan has at least two images")
        H0, W0 = _image_hw(images[0])
        self.rescale, self.crop = rescale, (None if crop is None else (int(crop[0]), int(crop[1])))
        _, _, _, _, H, W = ops.prep_geometry(H0, W0, rescale, self.crop)
        if H % 4 or W % 4:
            raise RuntimeError(f"ScanSession: the prepared size {W}x{H} must be a multiple of 4 (the cost volume lives at 1/4 resolution)")
        poses, intrinsics = torch.as_tensor(poses), torch.as_tensor(intrinsics)
        if tuple(poses.shape) != (M, 4, 4) or tuple(intrinsics.shape) != (M, 3, 3):
            raise ValueError(f"ScanSession: poses [M,4,4] and intrinsics [M,3,3] expected for M = {M} images")
        self.M, self.H, self.W, self.h, self.w = M, H, W, H // 4, W // 4
        need = self.bytes_needed(M, H, W)
        if max_bytes is not None and need > max_bytes:
            raise MemoryError(f"ScanSession: a scan of {M} images at {W}x{H} needs {need} bytes resident on the device "
                              f"({need / 2 ** 30:.2f} GiB), more than max_bytes = {max_bytes}; there is no partial store")
        self.encode_batch = max(1, int(encode_batch))
        # the projection matrices are formed on the host (projective.pij_matrices): poses and intrinsics stay there
        self.poses = poses.detach().to("cpu", torch.float32).clone()
        self.intrinsics = scan_intrinsics(intrinsics.detach().to("cpu", torch.float32), H0, W0, rescale, self.crop)
        self.timings = {}

        # ---- once per image: upload, prepare
        t0 = time.perf_counter()
        self.prepared = torch.empty(M, 3, H, W, device=dev, dtype=torch.float32)
        for i, im in enumerate(images):
            if _image_hw(im) != (H0, W0):
                raise ValueError(f"ScanSession: image {i} is not {W0}x{H0} like image 0")
            if im.dtype != torch.uint8:
                im = im.float()
            ops.image_prep(im.to(dev).contiguous(), rescale, self.crop, out=self.prepared[i], bgr=bgr and im.dtype == torch.uint8)
        torch.cuda.current_stream(dev).synchronize()
        self.timings["upload_prep_s"] = time.perf_counter() - t0

        self.pipe = DepthMapPipeline(core, streams=max(1, int(streams)))
        self.force_uncached = bool(force_uncached)
        self.store = None
        self._store_key = None
        self._store_ready = None
        self._slots = {}
        if self.cached and not calibrating(core):
            self._ensure_store()

    def __len__(self):
        return len(self.pipe)

    # ---- which path
    @property
    def cached(self):
        """True: depth maps run ``RAFT.forward_cached`` on the feature store; False: the ordinary forward on gathered stacks."""
        return not self.force_uncached and self.model.supports_cached(self.device)

    def _key(self):
        m = self.model
        return (m._params_sig(), bool(m._enc_f6))

    def _ensure_store(self):
        """(Re-)encode the store when the first model's parameters or encoder form are not the ones it was filled with."""
        key = self._key()
        if key == self._store_key:
            return
        m, dev = self.model, self.device
        self.pipe.synchronize()                        # (a re-encode must not overwrite blocks that forwards in flight still read)
        t0 = time.perf_counter()
        m._validate_packs()
        eng_f = m._get_engines(dev)[1]
        if self.store is None:                         # border texels are written once (zeros) and never touched again
            self.store = torch.zeros(self.M, (self.h + 4) * (self.w + 4), 128, device=dev, dtype=torch.float16)
        flag = ops.overflow_flag(dev)
        with torch.no_grad():
            for i0 in range(0, self.M, self.encode_batch):
                i1 = min(self.M, i0 + self.encode_batch)
                eng_f.features_split(self.prepared[i0:i1], None, self.store[i0:i1], n_ref=0, border=2, scale=0.125, raw=True, flag=flag)
        self._store_ready = torch.cuda.Event()
        self._store_ready.record(torch.cuda.current_stream(dev))
        self._store_key = key
        self._store_ready.synchronize()
        self.timings["encode_s"] = time.perf_counter() - t0

    def refresh_weights(self):
        """After the first model's parameters changed: copy them into the replicas; the store follows on the next depth map."""
        self.pipe.refresh_weights()

    def _slot_tensor(self, srcs):
        key = tuple(int(j) for j in srcs)
        t = self._slots.get(key)
        if t is None:
            if not key or min(key) < 0 or max(key) >= self.M:
                raise IndexError(f"ScanSession: source views {key} outside the scan of {self.M} images")
            t = self._slots[key] = torch.tensor(key, dtype=torch.int32, device=self.device)
        return t

    def stack(self, ref, srcs):
        """The stack the ordinary forward would get for this depth map: [1, 1+V, 3, H, W] gathered from the prepared images."""
        idx = torch.tensor([int(ref)] + [int(j) for j in srcs], device=self.device)
        return self.prepared.index_select(0, idx).unsqueeze(0)

    # ---- depth maps
    def submit(self, ref, srcs, scale):
        """Enqueue one depth map on the next stream; returns a handle for ``result``."""
        pipe, ref = self.pipe, int(ref)
        if not 0 <= ref < self.M:
            raise IndexError(f"ScanSession: reference view {ref} outside the scan of {self.M} images")
        srcs = [int(j) for j in srcs]
        _, m, st = pipe.pick()                          # (a replica still calibrating adopted the first model's form, or m is the first model)
        use_cached = self.cached and not calibrating(m)
        idx = [ref] + srcs
        poses, intr = self.poses[idx][None], self.intrinsics[idx][None]
        if use_cached:
            self._ensure_store()
            slots = self._slot_tensor(srcs)

        def forward():
            if use_cached:
                st.wait_event(self._store_ready)
                f1s = ops.feat_ref_rows(self.store[ref], self.h, self.w, border=2)
                return m.forward_cached(self.prepared[ref:ref + 1], f1s, self.store, slots, poses, intr, scale)
            # calibration pending, or a model whose forward does not take the direct-split path: the ordinary forward on a gathered stack
            return m(self.stack(ref, srcs), poses, intr, scale=scale)
        return pipe.launch(st, forward)

    def result(self, handle, wait_on_host=True):
        return self.pipe.result(handle, wait_on_host=wait_on_host)

    def depth(self, ref, srcs, scale):
        """[1,1,h,w] disparity * scale of reference view ``ref`` against source views ``srcs`` (best first), as ``RAFT.forward`` returns it."""
        return self.result(self.submit(ref, srcs, scale), wait_on_host=False)

    def depths(self, pairs, scales, num_frames=10):
        """One depth map per image i against ``pairs[i][:num_frames]`` with ``scales[i]`` -> float32 [M,h,w] on the device, ``len(self)`` depth maps
        in flight.  Each disparity is inverted on the stream that produced it (``ops.disp_to_depth``: ``inference.disp_to_depth``'s bits)
        straight into its slice.  The overflow protocol is the file drivers' (``pipeline.checked``); a ``SaturationError`` leaves nothing behind."""
        M = self.M
        if len(pairs) != M or len(scales) != M:
            raise ValueError(f"ScanSession.depths: pairs and scales need one entry per image ({M})")
        stack = torch.empty(M, self.h, self.w, device=self.device, dtype=torch.float32)
        cur = torch.cuda.current_stream(self.device)

        def inverted():
            for i in range(M):
                disp, _, st = self.submit(i, [int(j) for j in pairs[i]][:num_frames], scales[i])
                with torch.cuda.stream(st):
                    ops.disp_to_depth(disp, out=stack[i])
                    done = torch.cuda.Event()
                    done.record(st)
                yield done

        try:
            for _ in checked(self, self.model, inverted(), torch.cuda.Event.synchronize):
                pass
        finally:
            for st in self.pipe.streams:                    # (also on an error: no forward still writes into a stack that is let go)
                stack.record_stream(st)
                cur.wait_stream(st)
        return stack

    def synchronize(self):
        self.pipe.synchronize()

    def poll_overflow(self):
        return self.pipe.poll_overflow()

    def check_overflow(self, raise_error=True):
        return self.pipe.check_overflow(raise_error=raise_error)

    def close(self):
        self.pipe.synchronize()
        self.pipe.close()
        self.store = self.prepared = None
        self._store_key = None
        self._slots = {}


def inference_scan(model_or_ckpt, images, poses, intrinsics, names, pairs, scales, output_folder, rescale=1, crop=None, num_frames=10,
                   streams=3, write_min_depth=None, bgr=False, encode_batch=4, max_bytes=None, force_uncached=False, timings=None):
    """``inference()`` for a whole scan held in arrays: one depth map per image i with source views ``pairs[i][:num_frames]`` (best first, as
    the reference's load_pair orders them) and the loader's per-view ``scales[i]``; same files (``depths/{name}_scale{rescale}_nf{num_frames}.pfm``,
    the optional min-depth text), same overflow handling.  ``model_or_ckpt``: a RAFT, or a checkpoint path (None: untrained weights).
    ``timings``: a dict that receives the session's host-side figures.  Returns the list of files written."""
    output_folder = Path(output_folder)
    with running_model(model_or_ckpt) as core:
        (output_folder / "depths").mkdir(exist_ok=True, parents=True)
        sess = ScanSession(core, images, poses, intrinsics, rescale=rescale, crop=crop, streams=stream_count(core, streams),
                           encode_batch=encode_batch, max_bytes=max_bytes, bgr=bgr, force_uncached=force_uncached)
        try:
            M = sess.M
            if len(names) != M or len(pairs) != M or len(scales) != M:
                raise ValueError(f"inference_scan: names, pairs and scales need one entry per image ({M})")
            jobs = ((sess.submit(i, [int(j) for j in pairs[i]][:num_frames], scales[i]), names[i], num_frames) for i in range(M))
            return run_jobs(sess, core, jobs, output_folder, rescale, write_min_depth)
        finally:
            if timings is not None:
                timings.update(sess.timings)
                timings["cached"] = bool(sess.cached)
            sess.close()


def _depth_stacks(core, images, poses, intrinsics, pairs, scales, passes, num_frames, timings, **session_kw):
    """Step 1 of ``reconstruct_scan``: one session per pass, one after the other -> the depth stack [M,h,w] of every pass, and the colours
    and cameras of the first pass's images at the grid that is fused (the finer one in the two-pass form)."""
    stacks, colors, Ks, Es = [], None, None, None
    for k, s in enumerate(passes):
        sess = ScanSession(core, images, poses, intrinsics, rescale=s, **session_kw)
        try:
            stacks.append(sess.depths(pairs, scales, num_frames=num_frames))
            if k == 0:
                # colours and cameras as fusion() derives them from the prepared images and their intrinsics, at the grid that is fused
                gh, gw = (sess.h * 2, sess.w * 2) if len(passes) == 2 else (sess.h, sess.w)
                colors = FU.color_grid(sess.prepared, gh, gw)
                scale, flag, _, _, index = FU.depth_grid_geometry(sess.H, sess.W, gh, gw)
                Ks = torch.stack([FU.modify_camera_parameters(sess.intrinsics[i].clone().float(), scale, index, flag) for i in range(sess.M)])
                Es = sess.poses.clone().float()
                torch.cuda.current_stream(sess.device).synchronize()     # (the session's images go away with it)
            if timings is not None:
                timings.update(sess.timings)
                timings["cached"] = bool(sess.cached)
        finally:
            sess.close()
    return stacks, colors, Ks, Es


def _merged(stacks, colors, th, keep):
    """Step 2 of ``reconstruct_scan``, up to the vote loop: the stack that is fused (two passes: ``multires.merge`` per view, at the finer
    grid) and, with ``keep``, every pass's stack on the host for the PFMs."""
    if len(stacks) == 2:
        from .multires import merge
        if tuple(stacks[1].shape[1:]) != (colors.shape[2], colors.shape[3]):
            raise ValueError("reconstruct_scan: the second pass's depth grid is not twice the first's")
        depths = torch.stack([merge(stacks[0][i], stacks[1][i], th=th) for i in range(stacks[0].shape[0])])
    else:
        depths = stacks[0]
    torch.cuda.current_stream(depths.device).synchronize()
    return depths, ([st.cpu().numpy() for st in stacks] if keep else [])


def _cloud_tail(masks, est, Ks, Es, colors, refs, clean, normals, mesh=None):
    """Step 3 of ``reconstruct_scan``: masked pixels -> points and colours, the optional ``clean`` filter and ``normals`` (already checked
    options, or None) on the device, then the one copy to the host -> the result's arrays and the bytes that copy moved."""
    dev = masks.device
    if normals is None:
        xyz, rgb = FU.point_cloud(masks, est, Ks, Es, colors, refs)
    else:
        xyz, rgb, view_base = FU.point_cloud(masks, est, Ks, Es, colors, refs, view_base=True)
    out, kept = {}, None
    if mesh is not None:                                    # the grid is the fused cloud's, before ``clean`` thins it
        from .mesh import mesh_of_scan
        mv, mf, out["mesh_info"], attributes = mesh_of_scan(xyz, est, masks, Ks, Es, refs, mesh, colors=colors)
        out["mesh_vertices"], out["mesh_faces"] = mv.cpu().numpy(), mf.cpu().numpy()
        out.update({k: a.cpu().numpy() for k, a in attributes.items()})          # "mesh_colors" / "mesh_normals" / "mesh_sample*", if asked for
    if clean is not None:
        from .cloud_eval import clean_cloud
        kept, cleaned = clean_cloud(xyz, clean)
        out["clean"] = {"n_in": int(xyz.shape[0]), **cleaned}
        xyz, rgb = xyz.index_select(0, kept), rgb.index_select(0, kept)
    if normals is not None:
        from .cloud_eval import estimate_normals
        # the view of a fused row: the last k with view_base[k] <= row (views without a point share their base with the next one)
        rows = kept if kept is not None else torch.arange(int(xyz.shape[0]), device=dev)
        slot = torch.searchsorted(view_base, rows, right=True) - 1
        centres = FU.cloud_cams(Ks, Es)[:, [12, 16, 20]].float()[refs].to(dev)      # inv(E)[:3, 3] of every emitted view
        out["normal_info"] = {}
        nrm, _ = estimate_normals(xyz, viewpoints=centres.index_select(0, slot), info=out["normal_info"], **normals)
        out["normals"] = nrm.cpu().numpy()
    out.update(xyz=xyz.cpu().numpy(), rgb=rgb.cpu().numpy(), masks=masks.cpu().numpy().astype(bool), depth_est=est.cpu().numpy())
    nbytes = int(xyz.numel() * 4 + rgb.numel() + masks.numel() + est.numel() * 4)
    nbytes += sum(int(out[k].nbytes) for k in ("mesh_vertices", "mesh_faces", "mesh_colors", "mesh_normals", "mesh_samples", "mesh_sample_faces",
                                                 "mesh_sample_colors") if k in out)
    return out, nbytes + (int(out["normals"].nbytes) if normals is not None else 0)


def reconstruct_scan(model_or_ckpt, images, poses, intrinsics, names, pairs, scales, output_folder=None, rescale=1, crop=None, num_frames=10,
                     glb=0.25, streams=3, write_depths=False, write=True, th=0.02, bgr=False, encode_batch=4, max_bytes=None,
                     force_uncached=False, timings=None, clean=None, normals=None, mesh=None):
    """A scan to its fused point cloud without leaving the device between the stages: ``ScanSession.depths`` -> ``fusion.fuse_depth_maps`` (view i
    against ``pairs[i][:num_frames]``) -> ``fusion.point_cloud`` with the colours of ``fusion.color_grid``.  What ``inference_scan`` followed by
    ``fusion.fusion`` on the session's prepared images computes, without the PFM round trip, the host resize and the float64 numpy tail: same
    depth maps, masks and colours bit for bit, the points float32 roundings of the same fp64 arithmetic.  Arguments as ``inference_scan``;
    ``rescale=(s1, s2)`` with s2 = 2 s1 runs two sessions one after the other, merges the two depth stacks (``multires.merge(th=th)``) and fuses
    at the finer grid with the first session's images and cameras (no ``crop`` in that form).  ``write``: ``result.ply`` and ``mask/<i>.png`` under ``output_folder``;
    ``write_depths``: also the PFMs of ``inference_scan``, same names.  One device->host copy brings the cloud, the masks and the averaged
    depths back.  Returns ``fusion.fusion``'s dictionary (``xyz`` is float32 here).

    ``clean``: an outlier filter for the fused cloud (``cloud_eval.clean_cloud``), applied on the device between the fusion and
    that copy: {"method": "statistical", "k", "std_ratio", "max_dist"} (``remove_statistical_outliers``) or {"method": "radius", "radius",
    "min_neighbours"} (``remove_radius_outliers``).  ``xyz`` and ``rgb`` (and ``result.ply``) then hold the kept points in their fused order and
    the result gains "clean": {"n_in", "n_kept", and what the filter reports}; ``masks`` and ``depth_est`` stay as fused - a pixel whose point
    was filtered keeps its mask bit.  None (the default): no filter, no such key.

    ``normals``: True, or {"k", "max_dist", "cell"} for ``cloud_eval.estimate_normals`` (ValueError for another key): a surface
    normal for every point of the cloud as it leaves (after ``clean``), still on the device, turned towards the centre of the camera that
    produced the point - the one piece of information that orients a normal without guessing.  The result gains "normals" (float32 [n, 3];
    zeros where the neighbourhood has no plane) and "normal_info" ({"n_valid", "max_dist", "cell", "k"}), and ``result.ply`` carries nx ny nz.
    None (the default): no normals, no such keys, the file as before.

    ``mesh``: True, or {"voxel" | "resolution", "trunc", "min_weight", "margin"} (ValueError for another key): a surface through
    the fused depth maps, still on the device - ``mesh.grid_for`` around the fused cloud (before ``clean``), then ``mesh.mesh_from_depth_maps``
    over ``depth_est`` and the masks of the emitted views.  The result gains "mesh_vertices" (float32 [nv, 3]), "mesh_faces" (int32 [nf, 3])
    and "mesh_info" ({"grid", "trunc", "nv", "nf", "observed"}), and ``write`` puts ``result_mesh.ply`` beside ``result.ply``.  None (the
    default): no mesh, no such keys, no such file.  Two further keys of ``mesh``: "colors": True or {"tol": float} - a colour
    per vertex from the views that see it (``mesh.vertex_colors`` over the colour planes of the cloud; ``tol``, default the mesh's trunc, is
    the occlusion bound on |depth - uz|): the result gains "mesh_colors" (uint8 [nv, 3]) and ``mesh_info`` "coloured", the number of vertices
    some view sees; "normals": True - area-weighted vertex normals (``mesh.vertex_normals``): "mesh_normals" (float32 [nv, 3]).
    ``result_mesh.ply`` carries what was asked for.  Without these keys nothing changes.  And two: "min_component": n and
    "keep_largest": k, an int >= 1 each - ``mesh.remove_small_components`` right after the extraction: a connected piece stays iff it has at
    least n faces and is among the k largest; colours and normals are those of the returned mesh; ``mesh_info`` "nv" / "nf" describe it and
    it gains "extracted" (nv, nf before), "components", "removed_components", "removed_faces", "removed_vertices" and "sweeps".  And one
    (DESIGN.md 3zd): "simplify": k, a positive finite number - a clustering cell of k mesh voxels - or {"voxels": k | "cell": world units,
    "representative": "quadric" | "mean", "regularisation": float}: ``mesh.simplify_vertex_clustering`` after the small-piece removal and
    before colours and normals; ``mesh_info`` "nv" / "nf" describe the returned mesh and it gains "simplified_from" (nv, nf before),
    "clusters", "degenerate_faces", "duplicate_faces", "dropped_clusters" and "quadric".  And two: "smooth": n, an int
    >= 1 - Taubin smoothing with n iterations - or {"iterations": n, "method": "taubin" | "laplacian", "lam", "mu", "boundary": "fixed" |
    "free"}: ``mesh.smooth_mesh`` after the small-piece removal and before "simplify", colours and normals; ``mesh_info`` gains "smoothed"
    ({"moved", "frozen_boundary", "steps", "edges"}); "topology": True - ``mesh_info`` gains "topology", ``mesh.mesh_topology`` of the
    returned mesh.  And one: "fill_holes": n, an int >= 3 - ``mesh.fill_holes`` with ``max_edges`` = n: every boundary loop
    of at most n edges through simple vertices is closed, by one face (three edges) or by a fan around the loop's mean; it runs after the
    small-piece removal (an island's rim is a loop too) and before "smooth", "simplify", colours and normals; ``mesh_info`` "nv" / "nf"
    describe the returned mesh and it gains "filled" ({"holes", "added_vertices", "added_faces", "pinched_vertices",
    "boundary_edges_before"}).  Without the key nothing changes.  And one: "sample": n, an int >= 1, or {"n": samples |
    "density": samples per unit area | "spacing": world units, "seed": an int} with exactly one of the three - points on the surface of the
    returned mesh with a density proportional to area (``mesh.sample_mesh``; "spacing": ``mesh.sample_mesh_even``, thinned to that spacing).
    It runs last; the result gains "mesh_samples" (float32 [n, 3]), "mesh_sample_faces" (int32 [n], the face of every sample) and, when
    colours were asked for, "mesh_sample_colors" (uint8 [n, 3]); ``mesh_info`` gains "sampled", the call's info; ``write`` puts
    ``result_mesh_samples.ply`` beside ``result_mesh.ply``.  Without the key nothing changes."""
    two_pass = isinstance(rescale, (tuple, list))
    passes = [r for r in rescale] if two_pass else [rescale]
    if two_pass and (len(passes) != 2 or passes[1] != 2 * passes[0]):
        raise ValueError("reconstruct_scan: the two-pass form takes rescale=(s, 2 s)")
    if two_pass and crop is not None:
        raise ValueError("reconstruct_scan: the two-pass form takes no crop (the two passes would need windows that cover the same scene)")
    M = len(images)
    if len(names) != M or len(pairs) != M or len(scales) != M:
        raise ValueError(f"reconstruct_scan: names, pairs and scales need one entry per image ({M})")
    if (write or write_depths) and output_folder is None:
        raise ValueError("reconstruct_scan: writing needs an output_folder")
    if normals is not None:
        from .cloud_eval import normals_options
        normals = normals_options(normals)
    if mesh is not None:
        from .mesh import mesh_options
        mesh = mesh_options(mesh)
    t = {} if timings is None else timings
    # ---- 1. depth stacks, 2. merge and fuse
    tic = time.perf_counter()
    with running_model(model_or_ckpt) as core:
        stacks, colors, Ks, Es = _depth_stacks(core, images, poses, intrinsics, pairs, scales, passes, num_frames, timings, crop=crop,
                                               streams=stream_count(core, streams), encode_batch=encode_batch, max_bytes=max_bytes, bgr=bgr,
                                               force_uncached=force_uncached)
    depths, stacks_np = _merged(stacks, colors, th, keep=write_depths)
    del stacks                                              # (two-pass: the coarse and the fine stack are not needed behind the merge)
    t["depths_s"] = time.perf_counter() - tic
    tic = time.perf_counter()
    fpairs = [(i, [int(j) for j in pairs[i]][:num_frames]) for i in range(M)]
    masks, est, thre, hist = FU.fuse_depth_maps(depths, Ks, Es, fpairs, glb=glb)
    t["fuse_s"] = time.perf_counter() - tic
    # ---- 3. cloud tail
    tic = time.perf_counter()
    refs = [ref for ref, _ in fpairs]
    cloud, nbytes = _cloud_tail(masks, est, Ks, Es, colors, refs, clean, normals, mesh)
    t["d2h_bytes"] = nbytes + sum(int(a.nbytes) for a in stacks_np)
    # ---- 4. write
    if write_depths:
        (Path(output_folder) / "depths").mkdir(exist_ok=True, parents=True)
        for k, s in enumerate(passes):
            for i in range(M):
                write_pfm(depth_file(output_folder, names[i], s, num_frames), stacks_np[k][i])
    if write:
        FU.write_masks(Path(output_folder), cloud["masks"], refs)
        FU.write_ply(str(Path(output_folder) / "result.ply"), cloud["xyz"], cloud["rgb"], normals=cloud.get("normals"))
        if mesh is not None:
            from .mesh import write_mesh_ply
            write_mesh_ply(str(Path(output_folder) / "result_mesh.ply"), cloud["mesh_vertices"], cloud["mesh_faces"],
                           normals=cloud.get("mesh_normals"), colors=cloud.get("mesh_colors"))
            if "mesh_samples" in cloud:                     # a cloud: positions and the mixed vertex colours (black without colours)
                samples = cloud["mesh_samples"]
                FU.write_ply(str(Path(output_folder) / "result_mesh_samples.ply"), samples,
                             cloud.get("mesh_sample_colors", np.zeros((len(samples), 3), np.uint8)))
    t["tail_s"] = time.perf_counter() - tic
    out = {"masks": cloud["masks"], "depth_est": cloud["depth_est"], "xyz": cloud["xyz"], "rgb": cloud["rgb"], "threshold": thre, "history": hist}
    out.update({k: cloud[k] for k in ("clean", "normals", "normal_info", "mesh_vertices", "mesh_faces", "mesh_info", "mesh_colors", "mesh_normals",
                                     "mesh_samples", "mesh_sample_faces", "mesh_sample_colors") if k in cloud})
    return out
