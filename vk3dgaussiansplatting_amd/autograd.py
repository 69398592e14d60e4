"""Differentiable GS_RENDER_EXACT frames for PyTorch (include/gsplat.h, gs_backward*).

    r = make_renderer(width, height)                         # one context, reused frame after frame
    rgba = render(records, view, proj, cam_pos, sh_mode, renderer=r)            # float32 [H, W, 4]
    rgba, depth = render(records, ..., depth=True, renderer=r)                  # + float32 [H, W]

records: float32 [N, 84] on the renderer's GPU, in the record layout of ResourceManager.setGaussians.  The outputs are the
GS_OUTPUT_RGBA32F and GS_OUTPUT_DEPTH quantities of the frame (premultiplied colour before the clamp + 1 - T_end, blended
view depth); their backward is dL/d(records) from the library's HIP kernels.  The records reach the library through
gs_upload_gaussians_device (no host copy of the scene); the outputs come back through the host.

render(..., sparse_grad=True) returns dL/d(records) as a sparse COO tensor [N, 84] that lists only the splats the frame
rasterised (gs_backward_visible_device): no N-sized gradient is written, and torch.optim.SparseAdam moves only those rows.
It is meant for a leaf `records`.  torch's backward formulas of the ops a non-leaf `records` comes from (cat, slicing) do
not take sparse gradients, so a non-leaf input receives the same rows scattered into a dense [N, 84] tensor.

view, proj and cam_pos may be numpy arrays or torch tensors (any device, any float dtype); tensors that require grad receive
dL/dview, dL/dproj and dL/dcam_pos (gs_backward_camera_device, one call behind the record backward) for pose refinement.

    loss = photometric_loss(rgba, target, lambda_dssim=0.2, renderer=r)         # 0-dim: (1 - l) L1 + l (1 - SSIM)

photometric_loss is the library's fused L1 + D-SSIM (gs_photometric_loss_device): the three numbers and dloss/d(rgba) come
from one call on the device, and backward hands that gradient, times the upstream scalar, to the frame.

    opt = VisibleAdam(records, renderer=r)                                      # records: a plain tensor, updated in place
    numbers = opt.step(view, proj, cam_pos, sh_mode, target)                    # {loss, L1, DSSIM}, nothing waited for

VisibleAdam is the whole training step on the device: upload of the rows the last step moved, frame, loss, visible-row
gradients and an Adam step on those rows (gs_adam_rows_device), enqueued on one stream without a host wait.

    opt = VisibleAdam(records, renderer=r, track_density=True)                  # + gs_densify_stats_device in every step
    n_out, cloned, split, pruned = opt.densify(grad_threshold=2e-4)             # opt.records / m / v are the new cloud

    opt = VisibleAdam(records, renderer=r, space="raw")                         # Adam on log-scale, logit-opacity, raw rotation
    opt.reset_opacity(0.01); opt.save_ply("trained.ply")                        # the INRIA reset; a .ply gs_load_ply reads

    numbers = opt.step_batch(cameras, targets, sh_mode)                         # one Adam step on the mean loss of B views: [B, 3]

    opt.sh_degree = 0                                                           # the INRIA schedule: start at the DC term ...
    if it % 1000 == 0: opt.oneup_sh_degree()                                    # ... one degree up every 1000 iterations
    numbers = opt.step(view, proj, cam_pos, None, target)                       # sh_mode None: the mode of opt.sh_degree

    records, order = records_from_points(points, colors, renderer=r)            # a cloud from SfM points, in the loader's order

This module imports torch; `import vk3dgaussiansplatting_amd` does not import it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .renderer import FLOATS_PER_GAUSSIAN, Renderer, ResourceManager, default_adam_params, write_ply


def make_renderer(width: int, height: int, device: int = 0, **kw) -> Renderer:
    """A Renderer for render(): a context on `device` without a scene (the first render uploads one).  kw: Renderer's
    options (sort_algorithm, render_kernel, antialias, ...); render_mode must stay GS_RENDER_EXACT."""
    r = Renderer(width, height, device=device, record_timings=False, **kw)
    r.init(ResourceManager())
    return r


def _u32(n: int, dev, zero: bool = True) -> torch.Tensor:
    """n of the library's uint32 (ids, counts, marks) in int32 storage: every value here stays below 2^31, and a host
    copy is read with .view(np.uint32)."""
    return (torch.zeros if zero else torch.empty)(n, dtype=torch.int32, device=dev)


def _check_records(records: torch.Tensor, plain: bool = False):
    """records must be float32 [N, 84] on the GPU; plain: also contiguous and outside autograd, as VisibleAdam updates them."""
    if records.dtype != torch.float32 or records.dim() != 2 or records.shape[1] != FLOATS_PER_GAUSSIAN:
        raise ValueError(f"records must be float32 [N, {FLOATS_PER_GAUSSIAN}], not {records.dtype} {tuple(records.shape)}")
    if plain:
        if not records.is_cuda or not records.is_contiguous() or records.requires_grad:
            raise ValueError("records must be a contiguous tensor on the GPU that does not require grad")
    elif not records.is_cuda:
        raise ValueError("records must be on the GPU")


def _check_image(name: str, t: torch.Tensor, shape: tuple, apart: bool = False):
    """t must be float32 of `shape` ([H, W, C]) on the GPU; apart: a wrong shape or dtype and a host tensor are worded apart."""
    fits = t.dtype == torch.float32 and tuple(t.shape) == shape
    if apart:
        if not fits:
            raise ValueError(f"{name} must be float32 {shape}, not {t.dtype} {tuple(t.shape)}")
        if not t.is_cuda:
            raise ValueError(f"{name} must be on the GPU")
    elif not fits or not t.is_cuda:
        raise ValueError(f"{name} must be float32 {shape} on the GPU")


def _check_camera_grad(g: torch.Tensor, dev, one_of_many: bool = False):
    """g must be a contiguous float32 [35] tensor on dev: what gs_backward_camera_device fills."""
    if g.dtype != torch.float32 or tuple(g.shape) != (_lib.CAMERA_GRAD_FLOATS,) or g.device != dev or not g.is_contiguous():
        form = f"contiguous float32 [{_lib.CAMERA_GRAD_FLOATS}]"
        raise ValueError(f"camera_grads must hold {form} tensors on the records' device" if one_of_many else
                         f"camera_grad must be a {form} tensor on the records' device")


def _camera_array(x) -> np.ndarray:
    """A camera argument (numpy, a sequence, or a torch tensor on any device and of any float dtype) as the float32 host
    array the library takes."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, dtype=np.float32)


def _draw(r: Renderer, records: torch.Tensor, view, proj, cam_pos, sh_mode: int, want_depth: bool):
    """Upload records (device to device) and draw one frame; returns the host outputs."""
    torch.cuda.current_stream(records.device).synchronize()     # the library works on a stream of its own
    r.uploadDevice(records.data_ptr(), records.shape[0])
    r.ensureOutputs(_lib.GS_OUTPUT_RGBA32F | (_lib.GS_OUTPUT_DEPTH if want_depth else 0))
    r.drawCamera(view, proj, cam_pos, sh_mode)
    rgba = r.readOutput(_lib.GS_OUTPUT_RGBA32F)
    depth = r.readOutput(_lib.GS_OUTPUT_DEPTH) if want_depth else None
    return rgba, depth, r.frameSerial


class _Frame(torch.autograd.Function):
    @staticmethod
    def forward(ctx, records, renderer, view, proj, cam_pos, sh_mode, want_depth, sparse_grad):
        # tensor cameras that require grad receive gradients of their own shape, dtype and device (backward)
        ctx.cameras = [(tuple(t.shape), t.dtype, t.device) if isinstance(t, torch.Tensor) else None for t in (view, proj, cam_pos)]
        view, proj, cam_pos = _camera_array(view), _camera_array(proj), _camera_array(cam_pos)
        rgba, depth, frame = _draw(renderer, records, view, proj, cam_pos, sh_mode, want_depth)
        ctx.renderer, ctx.frame, ctx.args = renderer, frame, (view, proj, cam_pos, sh_mode, want_depth)
        ctx.sparse_grad = sparse_grad
        ctx.save_for_backward(records)
        out = torch.from_numpy(rgba).to(records.device)
        if want_depth:
            return out, torch.from_numpy(depth).to(records.device)
        return out

    @staticmethod
    def backward(ctx, grad_rgba, grad_depth=None):
        (records,) = ctx.saved_tensors
        r, dev, size = ctx.renderer, records.device, (records.shape[0], FLOATS_PER_GAUSSIAN)
        if r.frameSerial != ctx.frame:              # another frame was drawn since: draw this one again
            _draw(r, records.detach(), *ctx.args)
        g = (grad_rgba if grad_rgba is not None else torch.zeros(r.height, r.width, 4, device=dev))
        g = g.to(device=dev, dtype=torch.float32).contiguous()
        d = None
        if ctx.args[4] and grad_depth is not None:
            d = grad_depth.to(device=dev, dtype=torch.float32).contiguous()
        # one gs_backward_camera_device call behind the record backward, only when a camera tensor asks for its gradient
        cam = torch.zeros(_lib.CAMERA_GRAD_FLOATS, dtype=torch.float32, device=dev) if any(ctx.needs_input_grad[2:5]) else None
        # the row form is all that differs: every row of the cloud, or the rows of the splats the frame rasterised
        if ctx.sparse_grad:
            count = r.visibleCount()
            ids, seen = _u32(count, dev, zero=False), _u32(1, dev, zero=False)
            rows = torch.empty(count, FLOATS_PER_GAUSSIAN, dtype=torch.float32, device=dev)
            rows_form = (r.backwardVisibleDevice, ids.data_ptr() if count else None, rows.data_ptr() if count else None, count,
                         seen.data_ptr())
        else:
            count = records.shape[0]
            out = torch.empty(size, dtype=torch.float32, device=dev)
            rows_form = (r.backwardDevice, out.data_ptr())
        torch.cuda.current_stream(dev).synchronize()
        rows_form[0](g.data_ptr(), None if d is None else d.data_ptr(), *rows_form[1:])
        if cam is not None and count:               # a frame that rasterised nothing has no rows: the zeros stand
            r.backwardCameraDevice(cam.data_ptr())
        r.synchronize()
        if ctx.sparse_grad == "scatter":            # a non-leaf input
            out = torch.zeros(size, dtype=torch.float32, device=dev)
            out.index_copy_(0, ids.long(), rows)
        elif ctx.sparse_grad:
            out = torch.sparse_coo_tensor(ids.long()[None], rows, size=size)
        camera = (None, None, None)
        if cam is not None:
            camera = tuple(b.reshape(c[0]).to(device=c[2], dtype=c[1]) if c is not None and need else None
                           for b, c, need in zip((cam[0:16], cam[16:32], cam[32:35]), ctx.cameras, ctx.needs_input_grad[2:5]))
        return (out, None) + camera + (None, None, None)


def render(records: torch.Tensor, view, proj, cam_pos, sh_mode: int = 0, depth: bool = False, *, renderer: Renderer,
           sparse_grad: bool = False):
    """The frame of `records` (float32 [N, 84], CUDA/HIP, on the renderer's device) under the camera (view, proj: 4 x 4
    column-major as Camera.getViewMatrix / getProjectionMatrix give them, cam_pos: 3): rgba32f [H, W, 4], and depth [H, W]
    if asked, both differentiable w.r.t. records.  view, proj and cam_pos may also be torch tensors, on any device and of any
    float dtype: those that require grad receive dL/dview, dL/dproj, dL/dcam_pos in their own shape, dtype and device
    (gs_backward_camera_device, with its two conventions: the view's bottom row and the projection's clip-z row get 0);
    numpy cameras behave as before.  sparse_grad=True: records (meant to be a leaf) receives a sparse COO
    gradient over the splats the frame rasterised, with the values of the dense one; a non-leaf records receives those
    rows in a dense tensor."""
    _check_records(records)
    mode = ("sparse" if records.grad_fn is None else "scatter") if sparse_grad else None
    return _Frame.apply(records.contiguous(), renderer, view, proj, cam_pos, int(sh_mode), bool(depth), mode)


class _Loss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rgba, target, renderer, lam, bg):
        numbers = torch.empty(3, dtype=torch.float32, device=rgba.device)
        grad = torch.empty_like(rgba) if ctx.needs_input_grad[0] else None
        torch.cuda.current_stream(rgba.device).synchronize()        # the library works on a stream of its own
        renderer.photometricLossDevice(rgba.data_ptr(), target.data_ptr(), lam, bg, numbers.data_ptr(),
                                       None if grad is None else grad.data_ptr())
        renderer.synchronize()
        ctx.grad = grad
        return numbers[0].clone()

    @staticmethod
    def backward(ctx, upstream):
        return (None if ctx.grad is None else ctx.grad * upstream), None, None, None, None


def photometric_loss(rgba: torch.Tensor, target: torch.Tensor, lambda_dssim: float = 0.2, bg=None, *, renderer: Renderer):
    """(1 - lambda_dssim) * L1 + lambda_dssim * (1 - SSIM) of rgba (float32 [H, W, 4] on the renderer's GPU: the RGBA32F
    quantities, e.g. render()'s output) composited over bg (3 floats, None = black) against target (float32 [H, W, 3]), as a
    0-dim tensor, differentiable w.r.t. rgba.  H and W are the renderer's resolution; the renderer must hold a scene (any
    render() gives it one).  The definition is that of gs_photometric_loss in include/gsplat.h."""
    _check_image("rgba", rgba, (renderer.height, renderer.width, 4), apart=True)
    _check_image("target", target, (renderer.height, renderer.width, 3), apart=True)
    return _Loss.apply(rgba.contiguous(), target.detach().contiguous(), renderer, float(lambda_dssim), bg)


def records_from_points(points: torch.Tensor, colors: torch.Tensor | None = None, *, renderer: Renderer, **params):
    """The first records of a training run from a point cloud (gs_records_from_points_device) -> (records, order).

    points: float32 [n, 3] on the renderer's GPU, in the .ply's frame; colors: float32 [n, 3] in [0, 1], or None.  params:
    default_init_params()'s overrides (opacity, min_dist2, max_scale).  records: float32 [n, 84] in the loader's Morton
    order -- scale from the three nearest neighbours, identity rotation, SH DC from the colour; order: int64 [n], the input
    index of every row (records[k] is points[order[k]]).  Waits for the caller's stream before and for the renderer's
    after the call: a rare event.  For the trainer's parameters hand records to VisibleAdam(space="raw")."""
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 or not points.is_cuda:
        raise ValueError(f"points must be float32 [n, 3] on the GPU, not {points.dtype} {tuple(points.shape)}")
    if colors is not None and (colors.dtype != torch.float32 or colors.shape != points.shape or colors.device != points.device):
        raise ValueError("colors must be float32 [n, 3] on the points' device")
    p = _lib.default_init_params(**params)
    points = points.contiguous()
    colors = None if colors is None else colors.contiguous()
    n, dev = points.shape[0], points.device
    records = torch.empty(n, FLOATS_PER_GAUSSIAN, dtype=torch.float32, device=dev)
    order = _u32(n, dev, zero=False)
    torch.cuda.current_stream(dev).synchronize()                # the library works on a stream of its own
    renderer.recordsFromPointsDevice(points.data_ptr(), None if colors is None else colors.data_ptr(), n, p, records.data_ptr(),
                                     order.data_ptr())
    renderer.synchronize()
    return records, order.to(torch.int64)


class VisibleAdam:
    """Adam on the splats each frame rasterises, with the whole step on the device.

    records: float32 [N, 84] on the renderer's GPU, a plain tensor (no autograd); it is updated in place and stays the
    caller's.  The optimiser holds the moments m and v (zeros, like records), the ids / gradient rows / count a step lists
    (max_rows of them, N by default), the image-gradient buffer and the step counter; the library keeps no optimiser state.
    params: default_adam_params()'s overrides (lr, lo, hi per GS_ADAM_* group, beta1, beta2, eps).

    step() enqueues, on self.stream (a torch stream handed to the renderer with gs_set_stream): the upload of the records
    -- in full the first time, afterwards of the rows the previous step moved (gs_upload_rows_device reads the ids and
    count that step left) --, the frame, gs_photometric_loss_device on the context's own RGBA32F buffer,
    gs_backward_visible_device (and, with camera_grad, gs_backward_camera_device) and gs_adam_rows_device.  It waits for
    nothing: self.stream is made to follow the caller's
    current stream (so a target or records written there are seen), and the returned tensor {loss, L1, DSSIM} belongs to
    self.stream -- synchronise it, or make another stream wait for it, before the numbers are read.  Rows past max_rows
    are not updated (self.count holds |V| of the last step: compare after a synchronise).

    Between steps the caller may change records only in rows the last step listed, or must call reset_upload() so that
    the next step uploads everything.

    track_density=True: the optimiser also owns grad_accum, seen and max_radius (zeros of N), step() enqueues
    gs_densify_stats_device right behind the backward, and densify() replaces the cloud.

    abs_density=True (needs track_density): the AbsGS statistic beside the signed one.  The optimiser also owns
    grad_accum_abs (zeros of N), turns the renderer's setAbsGradients on, and enqueues gs_densify_stats_abs_device right
    behind gs_densify_stats_device, in step() and in every view of step_batch(); densify(abs_threshold=...) then splits by
    it.  Off (the default), the calls of a step are exactly those without it.

    space="raw": the optimiser moves self.raw -- log-scales, the logit of the opacity, the rotation before normalisation:
    the parameters a .ply stores, made from records by gs_raw_from_records_device -- and keeps records == act(raw) bit for
    bit (records is rewritten once, here, as act(raw): its scales and opacity move by the rounding of one log and one
    exp, its rotation becomes unit).  params default to default_adam_params(space="raw"): the INRIA rates, no clamps.
    step() is the same chain with gs_adam_rows_raw_device as its last call; reset_opacity() and save_ply() complete the
    trainer.  space="records" (the default) moves the record's own values.

    relocate(), grow() and add_noise() are the 3DGS-MCMC strategy (gs_relocate_device, gs_grow_device,
    gs_position_noise_device): dead splats moved onto live ones in place with no host wait and no new scene, the cloud grown
    to a cap, covariance-shaped noise on the positions.  They need no track_density.

    step_batch() is one step on several views: the visible rows of every view summed on the device
    (gs_rows_accumulate_device) and one Adam step on the union of their lists (gs_rows_collect_device)."""

    def __init__(self, records: torch.Tensor, *, renderer: Renderer, max_rows: int | None = None, track_density: bool = False,
                 space: str = "records", abs_density: bool = False, **params):
        _check_records(records, plain=True)
        if space not in ("records", "raw"):
            raise ValueError(f"space must be 'records' or 'raw', not {space!r}")
        if abs_density and not track_density:
            raise ValueError("abs_density=True needs track_density=True")
        self.records, self.renderer, self.space = records, renderer, space
        self.params = default_adam_params(space=space, **params)
        dev, n = records.device, records.shape[0]
        self.max_rows = n if max_rows is None else int(max_rows)
        self._rows_follow_n = max_rows is None
        self.track_density, self.abs_density = bool(track_density), bool(abs_density)
        if self.track_density:
            self._zero_stats(n, dev)
        self.m, self.v = torch.zeros_like(records), torch.zeros_like(records)
        self._alloc_rows(dev)
        self.acc = self.mark = None                       # step_batch's accumulator and marks: made on its first use
        self.grad = torch.zeros(renderer.height, renderer.width, 4, dtype=torch.float32, device=dev)
        self.t = 0
        self._full_upload = True
        self.stream = torch.cuda.Stream(device=dev)
        self.raw = torch.zeros_like(records) if space == "raw" else None
        torch.cuda.synchronize(dev)                       # the zeros above; gs_set_stream waits for the context's stream itself
        renderer.setStream(self.stream.cuda_stream)
        if self.abs_density:
            renderer.setAbsGradients(True)
        if space == "raw":
            self._raw_from_records()
            self.stream.synchronize()                     # once: records were rewritten, and the caller may read them anywhere

    def _raw_from_records(self):
        """self.raw <- the inverse of act on self.records, then self.records <- act(self.raw): from here on
        records == act(raw) bit for bit, which the chain of every step stands on.  On self.stream."""
        r, n = self.renderer, self.records.shape[0]
        r.rawFromRecordsDevice(self.records.data_ptr(), self.raw.data_ptr(), n)
        r.recordsFromRawDevice(self.raw.data_ptr(), self.records.data_ptr(), n)

    def _alloc_rows(self, dev):
        """What a step lists: ids and gradient rows (max_rows of them) and the count, all zero."""
        self.ids = _u32(self.max_rows, dev)
        self.rows = torch.zeros(self.max_rows, FLOATS_PER_GAUSSIAN, dtype=torch.float32, device=dev)
        self.count = _u32(1, dev)

    def _zero_stats(self, n: int, dev):
        self.grad_accum = torch.zeros(n, dtype=torch.float32, device=dev)
        self.seen = _u32(n, dev)
        self.max_radius = torch.zeros(n, dtype=torch.float32, device=dev)
        self.grad_accum_abs = torch.zeros(n, dtype=torch.float32, device=dev) if self.abs_density else None

    def _alloc_batch(self, dev):
        """What step_batch sums into: the accumulator (never initialised: a first touch is a store) and the zero marks."""
        n = self.records.shape[0]
        self.acc = torch.empty(n, FLOATS_PER_GAUSSIAN, dtype=torch.float32, device=dev)
        self.mark = _u32(n, dev)

    def _enqueue(self):
        """`with self._enqueue():` -- self.stream is made to follow the caller's current stream (so a target or records
        written there are seen) and is current inside the block: what the block allocates and enqueues belongs to it."""
        self.stream.wait_stream(torch.cuda.current_stream(self.records.device))
        return torch.cuda.stream(self.stream)

    def _upload_pending(self):
        """The records as the context must see them before a frame: in full the first time and after reset_upload(),
        afterwards the rows the previous step moved (gs_upload_rows_device reads the ids and count that step left)."""
        r, n = self.renderer, self.records.shape[0]
        if self._full_upload:
            r.uploadDevice(self.records.data_ptr(), n)             # a context without this scene: a new one (waits once)
            r.ensureOutputs(_lib.GS_OUTPUT_RGBA32F)
            self._full_upload = False
        else:
            r.uploadRowsDevice(self.records.data_ptr(), n, self.ids.data_ptr(), self.count.data_ptr(), self.max_rows)

    def _view(self, view, proj, cam_pos, sh_mode: int, target: torch.Tensor, numbers_ptr: int, lambda_dssim: float, bg,
              camera_grad: torch.Tensor | None):
        """One view's chain: the frame, gs_photometric_loss_device on the context's own RGBA32F buffer ({loss, L1, DSSIM}
        to numbers_ptr, the image gradient to self.grad), gs_backward_visible_device into self.ids / rows / count, with
        camera_grad gs_backward_camera_device, with track_density gs_densify_stats_device.  target and camera_grad may be
        the caller's own stream's: they are kept alive until self.stream is past them."""
        r = self.renderer
        target.record_stream(self.stream)
        r.drawCamera(view, proj, cam_pos, sh_mode, sync=False)
        r.photometricLossDevice(None, target.data_ptr(), float(lambda_dssim), bg, numbers_ptr, self.grad.data_ptr())
        r.backwardVisibleDevice(self.grad.data_ptr(), None, self.ids.data_ptr(), self.rows.data_ptr(), self.max_rows,
                                self.count.data_ptr())
        if camera_grad is not None:
            camera_grad.record_stream(self.stream)
            r.backwardCameraDevice(camera_grad.data_ptr())
        if self.track_density:
            r.densifyStatsDevice(self.ids.data_ptr(), self.count.data_ptr(), self.max_rows, self.records.shape[0],
                                 self.grad_accum.data_ptr(), self.seen.data_ptr(), self.max_radius.data_ptr())
            if self.abs_density:
                r.densifyStatsAbsDevice(self.ids.data_ptr(), self.count.data_ptr(), self.max_rows, self.records.shape[0],
                                        self.grad_accum_abs.data_ptr())

    def _adam(self):
        """t advanced once, then gs_adam_rows_device, or gs_adam_rows_raw_device in raw space, on self.ids / rows / count."""
        r, n = self.renderer, self.records.shape[0]
        self.t += 1
        self.params.step = self.t
        if self.space == "raw":
            r.adamRowsRawDevice(self.raw.data_ptr(), self.records.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), n,
                                self.ids.data_ptr(), self.rows.data_ptr(), self.count.data_ptr(), self.max_rows, self.params)
        else:
            r.adamRowsDevice(self.records.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), n, self.ids.data_ptr(),
                             self.rows.data_ptr(), self.count.data_ptr(), self.max_rows, self.params)

    def _resized(self):
        """After self.records / m / v (and raw) became tensors of another n, inside _enqueue: the density statistics start
        again from zero, ids, rows and max_rows follow the new size (a max_rows given to the constructor stays), and so do
        step_batch's buffers once they exist; then self.stream is waited for, and the next step uploads the whole cloud."""
        dev = self.records.device
        if self.track_density:
            self._zero_stats(self.records.shape[0], dev)
        if self._rows_follow_n:
            self.max_rows = self.records.shape[0]
        self._alloc_rows(dev)
        if self.acc is not None:
            self._alloc_batch(dev)
        self.stream.synchronize()
        # another n is another scene: the next step uploads everything and sets the resolution again (the output mask stays)
        self._full_upload = True

    def densify(self, abs_threshold: float | None = None, **params):
        """Clone, split and prune by the statistics gathered since the last call (gs_densify_device, params:
        default_densify_params()'s overrides) -> (n_out, cloned, split, pruned).
        abs_density=True: the AbsGS rule through the same call.  The accumulator handed to it is, per splat and in float32
        on the stream, smax > split_scale ? grad_accum_abs * (grad_threshold / abs_threshold) : grad_accum (smax: the
        largest of the record's three scales): large splats split by the mean ABSOLUTE screen gradient against
        abs_threshold, small ones clone by the signed mean against grad_threshold.  abs_threshold=None is 8e-4, the value
        AbsGS and gsplat's documentation publish: a hyper-parameter that nothing here has measured.  self.records, self.m and self.v become new
        tensors of n_out rows, the children beside their parents; the statistics start again from zero; ids, rows and max_rows
        follow the new size (a max_rows given to the constructor stays); the next step uploads the whole cloud as a new scene.
        t and the hyper-parameters stay.  Reading the four counts is the one host wait of this rare event.
        space="raw": density control runs on the records, then raw is made again from the new records and the records from
        that raw.  A kept row's raw value therefore moves by the rounding of one log and one exp -- far below a step, at a
        rare event -- and a split child starts from log(s / split_shrink)."""
        if not self.track_density:
            raise RuntimeError("VisibleAdam(track_density=True) gathers the statistics densify() goes by")
        if abs_threshold is not None and not self.abs_density:
            raise RuntimeError("VisibleAdam(abs_density=True) gathers the statistic abs_threshold goes by")
        p = _lib.default_densify_params(**params)
        r, dev, n = self.renderer, self.records.device, self.records.shape[0]
        with self._enqueue():
            accum = self.grad_accum
            if self.abs_density:
                ratio = float(np.float32(p.grad_threshold) / np.float32(8e-4 if abs_threshold is None else abs_threshold))
                large = self.records[:, 4:7].amax(dim=1) > float(p.split_scale)
                accum = torch.where(large, self.grad_accum_abs * ratio, self.grad_accum)
            out = [torch.empty(2 * n, FLOATS_PER_GAUSSIAN, dtype=torch.float32, device=dev) for _ in range(3)]
            counts = _u32(4, dev)
            r.densifyDevice(self.records.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), n, accum.data_ptr(),
                            self.seen.data_ptr(), self.max_radius.data_ptr(), p, out[0].data_ptr(), out[1].data_ptr(),
                            out[2].data_ptr(), 2 * n, counts.data_ptr())
            n_out, cloned, split, pruned = (int(x) for x in counts.cpu().numpy().view(np.uint32))      # waits for the stream
            if n_out == 0:
                raise RuntimeError("densify() would prune every gaussian")
            self.records, self.m, self.v = (t[:n_out].clone() for t in out)
            if self.space == "raw":
                self.raw = torch.zeros_like(self.records)
                self._raw_from_records()
            self._resized()
        return n_out, cloned, split, pruned

    def prune_by_contribution(self, cameras, threshold: float, sh_mode: int | None = None):
        """Drop every gaussian whose largest blend weight w = T * alpha over the given views stays below threshold
        (gs_contrib_device per view, then gs_prune_below_device with score = wmax) -> (n_out, dropped).

        cameras: a sequence of (view, proj, cam_pos); sh_mode as in step().  On self.stream: the pending upload (in full, or
        the rows the last step moved), then per view a frame and its contributions into zeroed self.wmax / self.wsum /
        self.pixels (float32 / float32 / uint32-in-int32 of the OLD n: they stay readable until the next call), with no loss
        and no optimiser step; then the kept rows of records, m, v and (space="raw") raw copied bit for bit, in order, into
        new tensors -- raw makes no log/exp round trip, unlike densify().  The density statistics start again from zero;
        ids, rows and max_rows follow the new size (a max_rows given to the constructor stays); the next step uploads the
        whole cloud as a new scene.  t and the hyper-parameters stay.  Reading the two counts is the one host wait.
        threshold has no default: no good value has been measured; the smallest positive float drops exactly the splats no
        view shows, which leaves the frames of these views bit for bit as they were while no list overflows."""
        cameras = list(cameras)
        if not cameras:
            raise ValueError("prune_by_contribution needs at least one camera")
        r, dev, n = self.renderer, self.records.device, self.records.shape[0]
        sh_mode = self.frame_sh_mode(sh_mode)
        with self._enqueue():
            self._upload_pending()
            self.wmax = torch.zeros(n, dtype=torch.float32, device=dev)
            self.wsum = torch.zeros(n, dtype=torch.float32, device=dev)
            self.pixels = _u32(n, dev)
            for view, proj, cam_pos in cameras:
                r.drawCamera(view, proj, cam_pos, sh_mode, sync=False)
                r.contribDevice(n, self.wmax.data_ptr(), self.wsum.data_ptr(), self.pixels.data_ptr())
            raw = self.space == "raw"
            out = [torch.empty(n, FLOATS_PER_GAUSSIAN, dtype=torch.float32, device=dev) for _ in range(4 if raw else 3)]
            counts = _u32(2, dev)
            r.pruneBelowDevice(self.wmax.data_ptr(), float(threshold), n, self.records.data_ptr(),
                               self.raw.data_ptr() if raw else None, self.m.data_ptr(), self.v.data_ptr(), out[0].data_ptr(),
                               out[3].data_ptr() if raw else None, out[1].data_ptr(), out[2].data_ptr(), n, counts.data_ptr())
            n_out, dropped = (int(x) for x in counts.cpu().numpy().view(np.uint32))      # waits for the stream
            if n_out == 0:
                raise RuntimeError("prune_by_contribution() would prune every gaussian")
            self.records, self.m, self.v = (t[:n_out].clone() for t in out[:3])
            if raw:
                self.raw = out[3][:n_out].clone()
            self._resized()
        return n_out, dropped

    # -- MCMC (3DGS-MCMC; include/gsplat.h, gs_relocate_device / gs_grow_device / gs_position_noise_device)
    # seed=None of the three methods is self.t with the call's own number in the upper word: the random words of relocate(),
    # grow() and add_noise() of one iteration are then different streams (the hash mixes the upper word in separately)
    _SEED_RELOCATE, _SEED_GROW, _SEED_NOISE = 0, 1 << 32, 2 << 32
    relocated = None       # relocate(): {changed, dead, sources} of the last call, on the device
    relocated_ids = None   # ... and the rows it changed, ascending (the first min(changed, n))

    def relocate(self, min_opacity: float = 0.005, seed: int | None = None):
        """Move every splat whose opacity is <= min_opacity onto a live one drawn in proportion to its opacity, in place
        (gs_relocate_device), opacity and scales of every copy corrected so that the picture stays; the moments of the changed
        rows start again from zero.  On self.stream: the pending upload, the call, then gs_upload_rows_device with the call's
        own ids and count -- n, the scene, the resolution and the scratch stay.  Nothing is waited for: self.relocated is the
        device tensor {changed, dead, sources}, self.relocated_ids the changed rows.  seed=None: self.t."""
        r, dev, n = self.renderer, self.records.device, self.records.shape[0]
        with self._enqueue():
            self._upload_pending()
            if self.relocated_ids is None or self.relocated_ids.shape[0] != n:
                self.relocated_ids = _u32(n, dev)
            self.relocated = _u32(3, dev)
            r.relocateDevice(self.records.data_ptr(), self.raw.data_ptr() if self.space == "raw" else None, self.m.data_ptr(),
                             self.v.data_ptr(), n, min_opacity, self.t | self._SEED_RELOCATE if seed is None else seed, self.relocated_ids.data_ptr(),
                             n, self.relocated.data_ptr())
            r.uploadRowsDevice(self.records.data_ptr(), n, self.relocated_ids.data_ptr(), self.relocated.data_ptr(), n)

    def grow(self, n_add: int | None = None, cap_max: int | None = None, factor: float = 1.05, min_opacity: float = 0.005,
             seed: int | None = None):
        """Grow the cloud by n_add rows (gs_grow_device) -> (n_out, sources): n_add live splats drawn in proportion to their
        opacity, the copies beside their sources with the relocation values and zero moments, every other row copied bit for
        bit.  n_add=None: min(cap_max, int(factor * n)) - n (cap_max=None: no cap).  self.records, self.m, self.v and
        (space="raw") self.raw become new tensors -- raw travels through the call, no log/exp round trip --; the rest is
        densify()'s bookkeeping: the next step uploads the whole cloud as a new scene, t and the hyper-parameters stay.
        Reading the two counts is the one host wait of this rare event.  seed=None: self.t + 2^32, not relocate()'s stream."""
        r, dev, n = self.renderer, self.records.device, self.records.shape[0]
        if n_add is None:
            target = int(factor * n)
            n_add = (target if cap_max is None else min(int(cap_max), target)) - n
        n_add = max(int(n_add), 0)
        raw = self.space == "raw"
        with self._enqueue():
            out = [torch.empty(n + n_add, FLOATS_PER_GAUSSIAN, dtype=torch.float32, device=dev) for _ in range(4 if raw else 3)]
            counts = _u32(2, dev)
            r.growDevice(self.records.data_ptr(), self.raw.data_ptr() if raw else None, self.m.data_ptr(), self.v.data_ptr(), n,
                         min_opacity, self.t | self._SEED_GROW if seed is None else seed, n_add, out[0].data_ptr(),
                         out[3].data_ptr() if raw else None, out[1].data_ptr(), out[2].data_ptr(), n + n_add, counts.data_ptr())
            n_out, sources = (int(x) for x in counts.cpu().numpy().view(np.uint32))      # waits for the stream
            self.records, self.m, self.v = (t if n_out == t.shape[0] else t[:n_out].clone() for t in out[:3])
            if raw:
                self.raw = out[3] if n_out == out[3].shape[0] else out[3][:n_out].clone()
            self.relocated_ids = None
            self._resized()
        return n_out, sources

    def add_noise(self, noise_lr: float, all_rows: bool = False, seed: int | None = None):
        """3DGS-MCMC exploration noise (gs_position_noise_device) with scale = noise_lr * lr[GS_ADAM_POSITION], on the rows the
        last step listed -- the next step's upload covers exactly those -- or, all_rows=True, on every row, followed by
        reset_upload().  Nothing is waited for.  seed=None: self.t + 2^33."""
        r, n = self.renderer, self.records.shape[0]
        scale = float(noise_lr) * float(self.params.lr[_lib.GS_ADAM_POSITION])
        seed = self.t | self._SEED_NOISE if seed is None else seed
        raw = self.raw.data_ptr() if self.space == "raw" else None
        with self._enqueue():
            if all_rows:
                r.positionNoiseDevice(self.records.data_ptr(), raw, n, None, None, 0, scale, seed=seed)
            else:
                r.positionNoiseDevice(self.records.data_ptr(), raw, n, self.ids.data_ptr(), self.count.data_ptr(), self.max_rows,
                                      scale, seed=seed)
        if all_rows:
            self.reset_upload()

    # The INRIA schedule's active SH degree: a trainer starts at 0 and calls oneup_sh_degree() every 1000 iterations.  The
    # default 3 (all 16 coefficients) is what a step drew before the degree existed.
    sh_degree = 3

    def oneup_sh_degree(self) -> int:
        """Raise the active SH degree by one, up to 3 -> the new degree."""
        self.sh_degree = min(int(self.sh_degree) + 1, 3)
        return self.sh_degree

    def frame_sh_mode(self, sh_mode: int | None = None) -> int:
        """The sh_mode a step draws with: an explicit integer as it is, None = the mode of self.sh_degree
        (gs_sh_mode_of_degree).  Host arithmetic: no context."""
        return _lib.sh_mode_of_degree(self.sh_degree) if sh_mode is None else int(sh_mode)

    def reset_upload(self):
        """The next step uploads every record (after the caller changed rows the last step did not list)."""
        self._full_upload = True

    def step(self, view, proj, cam_pos, sh_mode: int | None, target: torch.Tensor, lambda_dssim: float = 0.2, bg=None,
             camera_grad: torch.Tensor | None = None) -> torch.Tensor:
        """sh_mode: a GS_SH_* integer, or None for the mode of self.sh_degree (frame_sh_mode).
        camera_grad: a float32 [35] tensor on the records' device, filled with dL/dview, dL/dproj, dL/dcam_pos of this
        step's frame (gs_backward_camera_device) in the same enqueue chain, with no host wait; it belongs to self.stream
        like the returned numbers.  Needs max_rows > 0."""
        sh_mode = self.frame_sh_mode(sh_mode)
        if camera_grad is not None:
            _check_camera_grad(camera_grad, self.records.device)
        _check_image("target", target, (self.renderer.height, self.renderer.width, 3))
        target = target.contiguous()
        with self._enqueue():
            numbers = torch.empty(3, dtype=torch.float32, device=self.records.device)
            self._upload_pending()
            self._view(view, proj, cam_pos, sh_mode, target, numbers.data_ptr(), lambda_dssim, bg, camera_grad)
            self._adam()
        return numbers

    def step_batch(self, cameras, targets, sh_mode: int | None = None, lambda_dssim: float = 0.2, bg=None, weights=None,
                   camera_grads=None) -> torch.Tensor:
        """One Adam step on the weighted sum of the gradients of B views -> float32 [B, 3], {loss, L1, DSSIM} per view.
        sh_mode: a GS_SH_* integer, or None for the mode of self.sh_degree (frame_sh_mode).

        cameras: a sequence of (view, proj, cam_pos); targets: as many float32 [H, W, 3] tensors; weights: B floats, 1 / B
        each by default (the mean of the losses); camera_grads: None, or B float32 [35] tensors (the rows of a [B, 35]
        tensor serve), camera_grads[b] filled with the pose gradient of view b's own, unweighted loss.  One enqueue chain on
        self.stream with no host wait: the upload (in full the first time, afterwards the rows of the previous step's
        list, here the union), then per view the frame, the loss, gs_backward_visible_device into self.ids / rows / count
        (with camera_grads gs_backward_camera_device, with track_density gs_densify_stats_device: seen counts views) and
        gs_rows_accumulate_device into self.acc / self.mark; one gs_rows_collect_device back into self.ids / rows / count,
        the ascending union; one gs_adam_rows[_raw]_device with t advanced once.  With B = 1 and weights = [1.0] it moves
        records, m and v exactly as step() does.  max_rows bounds every view's list and the union; self.count holds the
        size of the union afterwards.  The returned tensor belongs to self.stream, as step()'s does."""
        r, n, dev = self.renderer, self.records.shape[0], self.records.device
        B = len(cameras)
        sh_mode = self.frame_sh_mode(sh_mode)
        if B == 0 or len(targets) != B:
            raise ValueError("step_batch needs at least one camera and a target for each")
        weights = [1.0 / B] * B if weights is None else [float(w) for w in weights]
        if len(weights) != B:
            raise ValueError(f"weights must have {B} entries")
        if camera_grads is not None:
            if len(camera_grads) != B:
                raise ValueError(f"camera_grads must have {B} entries")
            for g in camera_grads:
                _check_camera_grad(g, dev, one_of_many=True)
        shape = (r.height, r.width, 3)
        for target in targets:
            _check_image("every target", target, shape)
        targets = [t.contiguous() for t in targets]
        with self._enqueue():
            numbers = torch.empty(B, 3, dtype=torch.float32, device=dev)
            if self.acc is None:
                self._alloc_batch(dev)
            self._upload_pending()
            for b, ((view, proj, cam_pos), target) in enumerate(zip(cameras, targets)):
                self._view(view, proj, cam_pos, sh_mode, target, numbers[b].data_ptr(), lambda_dssim, bg,
                           None if camera_grads is None else camera_grads[b])
                r.rowsAccumulateDevice(self.acc.data_ptr(), self.mark.data_ptr(), n, self.ids.data_ptr(), self.rows.data_ptr(),
                                       self.count.data_ptr(), self.max_rows, weights[b])
            r.rowsCollectDevice(self.acc.data_ptr(), self.mark.data_ptr(), n, self.ids.data_ptr() if self.max_rows else None,
                                self.rows.data_ptr() if self.max_rows else None, self.max_rows, self.count.data_ptr())
            self._adam()
        return numbers

    def reset_opacity(self, max_opacity: float = 0.01):
        """The INRIA opacity reset (space="raw" only; gs_reset_opacity_raw_device): every opacity above max_opacity goes back
        to it, in records and as its logit in raw, and the opacity's moments of every row start again from zero.  The next
        step uploads the whole cloud.  Nothing is waited for."""
        if self.space != "raw":
            raise RuntimeError("reset_opacity() needs VisibleAdam(space='raw'); in record space clamp records[:, 15] and call reset_upload()")
        with self._enqueue():
            self.renderer.resetOpacityRawDevice(self.raw.data_ptr(), self.records.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                                self.records.shape[0], max_opacity)
        self.reset_upload()

    def save_ply(self, path: str):
        """The cloud as a .ply the loader reads (gs_write_ply).  space="raw": the raw rows as they are, so the file holds
        the trained parameters exactly; space="records": log and logit of the records.  Waits for self.stream and copies
        the rows to the host."""
        self.stream.synchronize()
        rows = self.raw if self.space == "raw" else self.records
        write_ply(path, rows.cpu().numpy(), self.space)
