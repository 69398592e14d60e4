"""Which Renderer calls a trainer method of autograd.py enqueues, in what order and with which arguments: VisibleAdam's constructor,
step, step_batch, densify, prune_by_contribution and reset_opacity in record space and in raw space, an optimiser with a fixed
max_rows and one with max_rows = 0, and render() + backward in its four row forms -- on the 64 gaussians at 32 x 32 (2 x 2 tiles) of
tests/test_call_sequences_gpu.py under two cameras (39 and 33 listed splats, 28 in both), against the committed list
tests/golden/trainer_calls.json.  The results of these methods are pinned bit for bit elsewhere (test_adam_gpu, test_batch_gpu,
test_densify_gpu, test_contrib_gpu, test_raw_gpu, ...); this file pins the calls themselves.

Every public method of the one Renderer instance is wrapped, as an instance attribute, by a logger that delegates;
torch.cuda.synchronize and torch.cuda.Stream.synchronize are logged while a trainer method runs.  A logged call is [name, arguments,
keyword arguments]: numbers, None and bools as they are; a device address as the name of the live tensor whose storage holds it
(the optimiser's attributes first, then the scenario's tensors) plus its byte offset; any other address local0, local1, ... by
first appearance inside that trainer method; a camera array by its camera; a GsAdamParams as its step.

The committed list was recorded with this file from the package of the commit before VisibleAdam's chain, resize and argument
checks were written once as helpers: GS_TRAINER_CALLS_RECORD=1 pytest tests/test_trainer_calls_gpu.py writes it (record_golden
below) instead of comparing."""
import contextlib
import json
import os

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib, synth
from conftest import ROOT

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "trainer_calls.json")
N, W, H = 64, 32, 32
POSES = (((0.0, 0.0, 0.0), 0.0, 0.0), ((0.3, 0.0, 0.0), 0.25, 0.0))


def cameras():
    """[(view, proj, cam_pos)] of cam0 and cam1."""
    out = []
    for pos, yaw, pitch in POSES:
        cam = gs.Camera(W / H)
        cam.setPosition(pos)
        cam.setRotation(yaw, pitch)
        cam.recalculate()
        out.append((cam.getViewMatrix().copy(), cam.getProjectionMatrix().copy(), cam.getPosition().copy()))
    return out


class Recorder:
    """The log of one Renderer: sections [label, calls], one per trainer method run inside method(label)."""

    running = None                                 # the recorder whose trainer method runs now: what the torch waits log into

    def __init__(self, renderer, cams):
        import torch
        self.torch, self.cams = torch, cams
        self.opt, self.tensors = None, {}          # whose attributes, and which other tensors, name a device address
        self.sections, self.calls, self.local = [], None, {}
        for name in dir(type(renderer)):
            if not name.startswith("_") and callable(getattr(renderer, name)):
                setattr(renderer, name, self.logged(name, getattr(renderer, name)))

    @classmethod
    def log_torch_waits(cls, monkeypatch):
        """torch.cuda.synchronize and torch.cuda.Stream.synchronize, logged into the running recorder."""
        import torch
        device_sync, stream_sync = torch.cuda.synchronize, torch.cuda.Stream.synchronize

        def synchronize(*args, **kw):
            if cls.running is not None:
                cls.running.calls.append(["torch.cuda.synchronize", [], {}])
            return device_sync(*args, **kw)

        def synchronize_stream(stream):
            rec = cls.running
            if rec is not None:
                mine = getattr(rec.opt, "stream", None) is not None and stream.cuda_stream == rec.opt.stream.cuda_stream
                rec.calls.append(["torch.cuda.Stream.synchronize", ["stream" if mine else "another stream"], {}])
            return stream_sync(stream)
        monkeypatch.setattr(torch.cuda, "synchronize", synchronize)
        monkeypatch.setattr(torch.cuda.Stream, "synchronize", synchronize_stream)

    def logged(self, name, fn):
        def call(*args, **kw):
            if self.calls is not None:
                self.calls.append([name, [self.spell(a) for a in args], {k: self.spell(v) for k, v in kw.items()}])
            return fn(*args, **kw)
        return call

    @contextlib.contextmanager
    def method(self, label):
        self.calls, self.local = [], {}
        Recorder.running = self
        try:
            yield self.calls
        finally:
            Recorder.running = None
            self.sections.append([label, self.calls])
            self.calls = None

    def result(self, values):
        self.sections[-1][1].append(["returned", [int(x) for x in values], {}])

    def named_tensors(self):
        own = sorted((k, v) for k, v in vars(self.opt).items() if isinstance(v, self.torch.Tensor)) if self.opt is not None else []
        return own + sorted(self.tensors.items())

    def spell(self, a):
        if a is None or isinstance(a, (bool, str)):
            return a
        if isinstance(a, (float, np.floating)):
            return float(a)
        if isinstance(a, _lib.GsAdamParams):
            return {"step": int(a.step)}
        if isinstance(a, _lib.GsDensifyParams):
            return "GsDensifyParams"
        if isinstance(a, np.ndarray):
            for k, cam in enumerate(self.cams):
                for part, x in zip(("view", "proj", "pos"), cam):
                    if a.shape == x.shape and np.array_equal(a, x):
                        return f"cam{k}.{part}"
            return f"array{list(a.shape)}"
        if isinstance(a, (int, np.integer)):
            a = int(a)
            if a < (1 << 32):
                return a
            for name, t in self.named_tensors():
                if t.is_cuda and t.untyped_storage().nbytes():
                    base = t.untyped_storage().data_ptr()
                    if base <= a < base + t.untyped_storage().nbytes():
                        return name if a == base else f"{name}+{a - base}"
            stream = getattr(self.opt, "stream", None) if self.opt is not None else None
            if stream is not None and a == stream.cuda_stream:
                return "stream.cuda_stream"
            return self.local.setdefault(a, f"local{len(self.local)}")
        return type(a).__name__


def recorded(cams):
    """A fresh renderer without a scene and its recorder."""
    from vk3dgaussiansplatting_amd.autograd import make_renderer
    r = make_renderer(W, H)
    return r, Recorder(r, cams)


def finish(r, rec):
    r.setStream(None)
    r.cleanup()
    return rec.sections


def new_optimiser(rec, r, aos, **kw):
    """VisibleAdam(...) with its constructor logged: the object exists before __init__ runs, so its attributes name addresses."""
    import torch
    from vk3dgaussiansplatting_amd.autograd import VisibleAdam
    records = torch.tensor(aos, device="cuda:0")
    torch.cuda.synchronize()
    rec.tensors["records_in"] = records
    rec.opt = VisibleAdam.__new__(VisibleAdam)
    with rec.method("constructor"):
        rec.opt.__init__(records, renderer=r, **kw)
    return rec.opt


def scenario_tensors(rec):
    import torch
    rng = np.random.default_rng(5)
    targets = [torch.tensor(rng.random((H, W, 3), dtype=np.float32), device="cuda:0") for _ in range(2)]
    cgrads = torch.zeros(2, _lib.CAMERA_GRAD_FLOATS, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    rec.tensors.update(target0=targets[0], target1=targets[1], cgrads=cgrads)
    return targets, cgrads


def trainer_scenario(aos, cams, space):
    r, rec = recorded(cams)
    targets, cgrads = scenario_tensors(rec)
    opt = new_optimiser(rec, r, aos, track_density=True, space=space)
    cam0, cam1 = cams
    with rec.method("step: full upload, the mode of degree 3"):
        opt.step(*cam0, None, targets[0])
    with rec.method("step: rows upload, camera_grad"):
        opt.step(*cam0, 0, targets[0], camera_grad=cgrads[0])
    with rec.method("step_batch: two views, camera_grads"):
        opt.step_batch([cam0, cam1], targets, camera_grads=[cgrads[0], cgrads[1]])
    opt.sh_degree = 0
    with rec.method("step: the mode of degree 0"):
        opt.step(*cam1, None, targets[1])
    n = opt.records.shape[0]
    with rec.method("densify"):
        counts = opt.densify(grad_threshold=0.0)
    rec.result(counts)
    assert counts[0] == opt.records.shape[0] > n
    n = counts[0]
    with rec.method("step_batch: full upload of the new n, weights"):
        opt.step_batch([cam0, cam1], targets, weights=[0.25, 0.75])
    with rec.method("prune_by_contribution"):
        kept = opt.prune_by_contribution([cam0, cam1], 1e-30)
    rec.result(kept)
    assert 0 < kept[0] < n and kept[0] == opt.records.shape[0] and kept[0] + kept[1] == n
    with rec.method("step: after the prune"):
        opt.step(*cam0, 0, targets[0])
    if space == "raw":
        with rec.method("reset_opacity"):
            opt.reset_opacity()
        with rec.method("step: after the reset"):
            opt.step(*cam0, 0, targets[0])
    opt.stream.synchronize()
    return finish(r, rec)


def fixed_rows_scenario(aos, cams):
    r, rec = recorded(cams)
    targets, _ = scenario_tensors(rec)
    opt = new_optimiser(rec, r, aos, max_rows=16, track_density=True)
    with rec.method("step"):
        opt.step(*cams[0], 0, targets[0])
    with rec.method("densify"):
        counts = opt.densify(grad_threshold=0.0)
    rec.result(counts)
    assert opt.max_rows == 16 and opt.ids.shape[0] == 16 and counts[0] > N
    opt.stream.synchronize()
    return finish(r, rec)


def no_rows_scenario(aos, cams):
    r, rec = recorded(cams)
    targets, _ = scenario_tensors(rec)
    opt = new_optimiser(rec, r, aos, max_rows=0)
    with rec.method("step_batch: the count-only collect"):
        opt.step_batch(cams, targets, 0)
    opt.stream.synchronize()
    return finish(r, rec)


def render_scenario(aos, cams):
    import torch
    from vk3dgaussiansplatting_amd.autograd import render
    r, rec = recorded(cams)
    view, proj, pos = cams[0]

    def leaf():
        t = torch.tensor(aos, device="cuda:0", requires_grad=True)
        torch.cuda.synchronize()
        rec.tensors = {"records": t}
        return t

    def backward(label, loss):
        with rec.method("backward: " + label):
            loss.backward()

    records = leaf()
    with rec.method("render: dense with depth"):
        rgba, depth = render(records, view, proj, pos, 0, depth=True, renderer=r)
    backward("dense with depth", rgba.sum() + depth.sum())
    assert records.grad.shape == (N, 84) and not records.grad.is_sparse

    records = leaf()
    with rec.method("render: sparse, a leaf"):
        rgba = render(records, view, proj, pos, 0, renderer=r, sparse_grad=True)
    backward("sparse, a leaf", rgba.sum())
    assert records.grad.is_sparse

    records = leaf()
    scaled = records * 1.0
    rec.tensors["scaled"] = scaled
    with rec.method("render: sparse, not a leaf"):
        rgba = render(scaled, view, proj, pos, 0, renderer=r, sparse_grad=True)
    backward("sparse, not a leaf", rgba.sum())
    assert not records.grad.is_sparse

    records = leaf()
    camera = [torch.tensor(x, requires_grad=True) for x in (view, proj, pos)]
    with rec.method("render: dense, camera tensors"):
        rgba = render(records, *camera, 0, renderer=r)
    backward("dense, camera tensors", rgba.sum())
    assert [tuple(c.grad.shape) for c in camera] == [(16,), (16,), (3,)]
    return finish(r, rec)


def record_golden(answers):
    """GS_TRAINER_CALLS_RECORD=1: writes the committed list."""
    with open(GOLDEN, "w") as f:
        json.dump(answers, f, indent=0, sort_keys=True)
        f.write("\n")


def test_trainer_methods_make_the_recorded_calls(monkeypatch):
    pytest.importorskip("torch")
    aos = np.ascontiguousarray(synth.generate(N, W, H, -3.0, seed=11), dtype=np.float32)
    cams = cameras()
    Recorder.log_torch_waits(monkeypatch)
    answers = {"records": trainer_scenario(aos, cams, "records"), "raw": trainer_scenario(aos, cams, "raw"),
               "max_rows 16": fixed_rows_scenario(aos, cams), "max_rows 0": no_rows_scenario(aos, cams),
               "render": render_scenario(aos, cams)}
    answers = json.loads(json.dumps(answers))
    # a training step waits for nothing: not for the device, not for a torch stream, not for the context's
    for piece, sections in answers.items():
        for label, calls in sections:
            if label.startswith("step"):
                assert not [c for c in calls if "synchronize" in c[0]], (piece, label)
    if os.environ.get("GS_TRAINER_CALLS_RECORD"):
        record_golden(answers)
        return
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(answers)
    for piece, sections in answers.items():
        assert [s[0] for s in sections] == [s[0] for s in golden[piece]], piece
        for (label, calls), (_, want) in zip(sections, golden[piece]):
            for k, (got, exp) in enumerate(zip(calls, want)):
                assert got == exp, (piece, label, k, got, exp)
            assert len(calls) == len(want), (piece, label, calls[len(want):], want[len(calls):])
