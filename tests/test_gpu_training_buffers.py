"""The caller-provided buffers of the training, grid, march and sampler wrappers of nerf_for_angiography_amd/engine.py, in the manner of
tests/test_gpu_engine_buffers.py (the helpers alone, on the host: tests/test_engine_buffers_cpu.py).  On the smallest shapes on which the
checks can go wrong - the smallest model the library admits (one hidden layer of width 64, as tests/exact_problems.py), 9 rays of 6
samples, 3 packed groups, a 5 x 3 x 7 grid (105 cells, 4 words: the ragged last word), n_draw 4, 2 batches of 3:

  acceptance  a call with every optional buffer passed returns the very tensors passed, and what it writes equals, bit for bit, what the
              call that allocates for itself returns; for an input that may be strided, the strided call equals the contiguous one;
  refusal     each buffer of the table in turn is given a wrong dtype of equal byte size, a non-contiguous view (buffers that are written,
              and the inputs that are never copied) and one element too few: a ValueError that names it, and every output buffer and
              grad_flat, painted beforehand, keep their bytes - nothing was launched.

Every wrong buffer is a view into an allocation at least as large as the right one (the short one the leading part of a full-size one),
so a refusal missed by mistake would still write only into memory this test owns.

Run with -m gpu on an MI355X."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
R, S, G, NF = 9, 6, 3, 2
RES, NC, WORDS, BOX = (5, 3, 7), 105, 4, [0.0, 0.0, 0.0, 5.0, 3.0, 7.0]
N_DRAW, N_BATCHES, K = 4, 2, 3
NEAR, FAR, STEP, EPS, THRE = 0.0, 9.0, 0.5, 1e-4, 1e-2
I32, I64, U8, F32, F64 = torch.int32, torch.int64, torch.uint8, torch.float32, torch.float64
SAME_SIZE = {I32: F32, F32: I32, I64: F64, F64: I64, U8: torch.int8}
ALL, NO_STRIDE, DTYPE = ("dtype", "strided", "short"), ("dtype", "short"), ("dtype",)


def _eng():
    from nerf_for_angiography_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _inputs():
    """The shared inputs, made once and never written to."""
    e = _eng()
    eng, eng_f = e.Engine(64, 1), e.Engine(64, 2, enc="fourier", n_freq=4)
    gen = torch.Generator().manual_seed(1)
    rnd = lambda *shape: torch.rand(*shape, generator=gen)
    flat = ((rnd(eng.param_count) - 0.5) * 0.4).to(DEV)
    prep = {p: eng.prepare(flat, None, p).clone() for p in ("f32", "f16s8")}
    o = torch.stack([torch.linspace(0.5, 4.5, R), torch.full((R,), 1.5), torch.full((R,), -1.0)], 1).to(DEV)
    d = torch.tensor([[0.0, 0.0, 1.0]]).repeat(R, 1).to(DEV)
    lens = torch.tensor([5, 32, 7] + [0] * (R - 3))
    off = torch.cat([torch.zeros(1, dtype=I64), torch.cumsum(lens, 0)]).to(DEV)
    ts = (1.0 + 0.1 * torch.arange(44)).to(DEV)
    packed = e.pack_groups(off, ts, ts + 0.1)
    assert packed.n_groups == G
    raw = (rnd(R, S) - 0.5).to(DEV)
    z = torch.linspace(1.5, 7.5, S).to(DEV)
    rgb = e.composite_dense(raw, d, z, want_aux=False)[0]
    ri = torch.arange(R, dtype=I32).repeat_interleave(S).to(DEV)
    torch.cuda.synchronize()
    return dict(eng=eng, eng_f=eng_f, flat=flat, flat_f=torch.zeros(eng_f.param_count, device=DEV), prep=prep, o=o, d=d, pts=o.clone(),
                tgt=torch.linspace(0.1, 0.9, R).to(DEV), z=z, u=rnd(R, NF).to(DEV), raw=raw, rgb=rgb, ri=ri, pred=raw.reshape(-1).clone(),
                bits=torch.tensor([-1, -1, -1, (1 << (NC - 96)) - 1], dtype=I32, device=DEV), off=off, ts=ts, packed=packed, goff=packed.group_offsets,
                w=(rnd(R) + 0.1).to(DEV), step=torch.zeros((), dtype=I64, device=DEV), idx=torch.tensor([1, 4, 7], device=DEV),
                acc=e.RenderSpec(R, S, origins=o, dirs=d, mode="acc", t_near=1.0, t_far=8.0),
                dense=e.RenderSpec(R, S, origins=o, dirs=d, mode="dense", z=z))


class Case:
    """One wrapper: `buffers` name -> (dtype, shape, the violations tried) of the caller buffers under test - `written` names those the
    wrapper writes (painted in the refusal test), `optional` those it allocates when they are not passed; `call(b)` takes the buffers of
    `b` in place of the valid ones and returns name -> tensor for the optional ones."""
    written, optional = (), ()

    def valid(self, name):
        """A valid, zero-filled stand-in for a written buffer (the read ones have theirs in _inputs())."""
        dtype, shape, _ = self.buffers[name]
        return torch.zeros(shape, dtype=dtype, device=DEV)

    def workspace(self):
        return None


def _nbytes(prec):
    return _inputs()["prep"][prec].numel()


class ModelCase(Case):
    """An Engine method that reads `prepared` (at self.prec) and adds to `grad_flat`."""
    prec, written, extra = "f16s8", ("grad_flat",), {}

    @property
    def buffers(self):
        return dict({"prepared": (U8, (_nbytes(self.prec),), NO_STRIDE), "grad_flat": (F32, (_inputs()["eng"].param_count,), ALL)}, **self.extra)

    def call(self, b):
        i = _inputs()
        return self.run(i, i["eng"], b.get("prepared", i["prep"][self.prec]), b["grad_flat"] if "grad_flat" in b else self.valid("grad_flat"), b)


class MlpBackward(ModelCase):
    prec = "f32"

    def run(self, i, eng, prep, grad, b):
        eng.mlp_backward(prep, i["pts"], i["tgt"], grad, "f32")


class MlpBackwardInputs(ModelCase):
    prec, written, extra = "f32", ("grad_flat", "d_pts"), {"d_pts": (F32, (R, 3), ALL)}

    def run(self, i, eng, prep, grad, b):
        eng.mlp_backward_inputs(prep, i["pts"], i["tgt"], grad, b.get("d_pts", self.valid("d_pts")), "f32")


class Infer(ModelCase):
    prec, written = "f32", ()

    @property
    def buffers(self):
        return {"prepared": (U8, (_nbytes("f32"),), NO_STRIDE)}

    def call(self, b):
        i = _inputs()
        return {"out": i["eng"].infer(b.get("prepared", i["prep"]["f32"]), b.get("points", i["pts"]), "f32")}


class RenderBackward(ModelCase):
    prec = "f32"

    def run(self, i, eng, prep, grad, b):
        eng.render_backward(prep, i["acc"], i["tgt"], i["tgt"], grad, "f32")


class RenderBackwardInputs(ModelCase):
    prec, written, extra = "f32", ("grad_flat", "d_origins", "d_dirs"), {"d_origins": (F32, (R, 3), ALL), "d_dirs": (F32, (R, 3), ALL)}

    def run(self, i, eng, prep, grad, b):
        eng.render_backward_inputs(prep, i["acc"], i["tgt"], i["tgt"], grad, b.get("d_origins", self.valid("d_origins")),
                                   b.get("d_dirs", self.valid("d_dirs")), "f32")


class TrainStep(ModelCase):
    def run(self, i, eng, prep, grad, b):
        spec = i["acc"] if "origins" not in b else _eng().RenderSpec(R, S, origins=b["origins"], dirs=i["d"], mode="acc", t_near=1.0, t_far=8.0)
        return {"pixel": eng.train_step_mse(prep, spec, b.get("target", i["tgt"]), 1.0 / R, grad, "f16s8"), "grad_flat": grad}


class HierTrainStep(ModelCase):
    def run(self, i, eng, prep, grad, b):
        eng.hier_train_step_mse(prep, i["dense"], NF, i["u"], i["tgt"], 1.0 / R, grad, "f16s8")


class TrainStepPacked(ModelCase):
    def run(self, i, eng, prep, grad, b):
        eng.train_step_packed_mse(prep, i["o"], i["d"], i["packed"], i["tgt"], 1.0 / R, grad, "f16s8")


class MarchStep(ModelCase):
    def run(self, i, eng, prep, grad, b):
        eng.march_train_step_mse(prep, i["o"], i["d"], i["tgt"], 1.0 / R, grad, "f16s8", BOX, NEAR, FAR, STEP, EPS, THRE, grid_bits=i["bits"],
                                 grid_aabb=BOX, grid_res=RES)


class MarchStepDeviceSizes(ModelCase):
    written, optional = ("grad_flat", "pixel", "counts", "skip"), ("pixel", "counts", "skip")
    extra = {"pixel": (F32, (R,), ALL), "counts": (I64, (3,), ALL), "skip": (F32, (1,), ALL)}

    def __init__(self, fn):
        self.fn = fn

    def run(self, i, eng, prep, grad, b):
        res = getattr(eng, self.fn)(prep, i["o"], i["d"], i["tgt"], 1.0 / R, grad, "f16s8", BOX, NEAR, FAR, STEP, EPS, THRE,
                                    grid_bits=b.get("grid_bits", i["bits"]), grid_aabb=BOX, grid_res=RES, pixel=b.get("pixel"),
                                    counts=b.get("counts"), skip=b.get("skip"))
        return dict(zip(("pixel", "counts", "skip"), res), grad_flat=grad)


class MarchStepBits(MarchStepDeviceSizes):
    """The march's bitfield, which may be longer than the grid needs."""
    buffers = {"grid_bits": (I32, (WORDS,), ALL)}
    written, optional = ("grad_flat",), ()


class CompositeDense(Case):
    buffers = {"dirs": (F32, (R, 3), NO_STRIDE), "z": (F32, (S,), NO_STRIDE)}

    def call(self, b):
        i = _inputs()
        return dict(zip(("rgb", "depth", "w", "ent", "sig"), _eng().composite_dense(b.get("raw", i["raw"]), b.get("dirs", i["d"]), b.get("z", i["z"]))))


class CompositeDenseBackward(Case):
    buffers = {"raw": (F32, (R, S), DTYPE), "dirs": (F32, (R, 3), NO_STRIDE), "z": (F32, (S,), NO_STRIDE), "rgb": (F32, (R,), NO_STRIDE),
               "d_rgb": (F32, (R,), NO_STRIDE)}

    def call(self, b):
        i = _inputs()
        _eng().composite_dense_backward(b.get("raw", i["raw"]), b.get("dirs", i["d"]), b.get("z", i["z"]), b.get("rgb", i["rgb"]), b.get("d_rgb", i["tgt"]))


class FineDepths(Case):
    buffers = {"z_coarse": (F32, (S,), NO_STRIDE), "u": (F32, (R, NF), NO_STRIDE)}

    def __init__(self, fn):
        self.fn = fn

    def call(self, b):
        i = _inputs()
        return {"out": getattr(_eng(), self.fn)(b.get("z_coarse", i["z"]), i["raw"].abs(), b.get("u", i["u"]))}


class Topk(Case):
    buffers = {"keys": (F32, (R,), DTYPE)}

    def call(self, b):
        return {"out": _eng().topk_indices(b.get("keys", _inputs()["w"]), K)}


class GatherRays(Case):
    buffers = {"origins": (F32, (R, 3), ALL), "dirs": (F32, (R, 3), ALL), "pixels": (F32, (R,), ALL), "idx": (I64, (K,), ("dtype", "strided")),
               "origins_out": (F32, (K, 3), ALL), "dirs_out": (F32, (K, 3), ALL), "pixels_out": (F32, (K,), ALL)}
    written = ("origins_out", "dirs_out", "pixels_out")

    def call(self, b):
        i = _inputs()
        outs = {k: b.get(k, self.valid(k)) for k in self.written}
        _eng().gather_rays(b.get("origins", i["o"]), b.get("dirs", i["d"]), b.get("pixels", i["tgt"]), b.get("idx", i["idx"]), **outs)
        return outs


class GridSelect(Case):
    buffers = {"bits": (I32, (WORDS,), ALL), "cells": (I32, (2 * N_DRAW,), ALL), "count": (I64, (1,), ALL)}
    written = optional = ("cells", "count")

    def workspace(self):
        return _eng().grid_select_workspace_bytes(BOX, RES)

    def call(self, b):
        res = _eng().grid_select_cells(BOX, RES, b.get("bits", _inputs()["bits"]), N_DRAW, 3, 5, b.get("cells"), b.get("count"), b.get("workspace"))
        return dict(zip(("cells", "count"), res))

    def specified(self, res):
        return dict(res, cells=res["cells"][:int(res["count"])])       # (slots behind the count are unwritten)


class GridRefresh(Case):
    written = ("occs", "binary_u8", "bits")

    @property
    def buffers(self):
        return {"prepared": (U8, (_nbytes("f16s8"),), NO_STRIDE), "occs": (F32, (NC,), ALL), "binary_u8": (U8, (NC,), ALL), "bits": (I32, (WORDS,), ALL)}

    def workspace(self):
        return _eng().grid_refresh_workspace_bytes(BOX, RES, N_DRAW, False)

    def call(self, b):
        i = _inputs()
        ws = b["workspace"] if "workspace" in b else torch.empty(self.workspace(), dtype=U8, device=DEV)
        _eng().grid_refresh(i["eng"], b.get("prepared", i["prep"]["f16s8"]), "f16s8", BOX, RES, b.get("occs", self.valid("occs")),
                            b.get("binary_u8", self.valid("binary_u8")), b.get("bits", self.valid("bits")), N_DRAW, False, 3, 5, 1e-2, 0.95, ws)


class SampleBatches(Case):
    buffers = {"weights": (F32, (R,), DTYPE), "out_idx": (I64, (N_BATCHES, K), ALL)}
    written = optional = ("out_idx",)

    def workspace(self):
        return _eng().sample_batches_workspace_bytes(R, N_BATCHES)

    def call(self, b):
        i = _inputs()
        return {"out_idx": _eng().sample_batches_dev(b.get("weights", i["w"]), 7, i["step"], N_BATCHES, K, b.get("out_idx"), b.get("workspace"))}


class EncodingGrad(Case):
    @property
    def buffers(self):
        return {"flat": (F32, (_inputs()["eng_f"].param_count,), ALL), "d_aux": (F32, (12,), ALL)}

    def call(self, b):
        i = _inputs()
        with i["eng_f"].encoding_grad(b.get("flat", i["flat_f"]), b.get("d_aux", torch.zeros(12, device=DEV))):
            pass


class PackGroups(Case):
    buffers = {"offsets": (I64, (R + 1,), ("dtype", "strided")), "group_offsets": (I64, (R + 1,), ALL)}

    def call(self, b):
        i = _inputs()
        _eng().pack_groups(b.get("offsets", i["off"]), i["ts"], i["ts"] + 0.1, G, b.get("group_offsets", i["goff"]))


class EntropyBackward(Case):
    written = optional = ("out",)

    def __init__(self, dense):
        self.dense = dense
        self.buffers = {"out": (F32, (R, S) if dense else (R * S,), ALL)}

    def call(self, b):
        e, i = _eng(), _inputs()
        if self.dense:
            sums = e.ray_entropy_dense(i["raw"], i["rgb"])[1]
            return {"out": e.ray_entropy_dense_backward(i["raw"], i["rgb"], sums, i["tgt"], out=b.get("out"))}
        sums = e.ray_entropy_packed(i["pred"], i["ri"], i["rgb"], R)[1]
        return {"out": e.ray_entropy_packed_backward(i["pred"], i["ri"], i["rgb"], sums, i["tgt"], out=b.get("out"))}


CASES = {"mlp_backward": MlpBackward(), "mlp_backward_inputs": MlpBackwardInputs(), "infer": Infer(), "render_backward": RenderBackward(),
         "render_backward_inputs": RenderBackwardInputs(), "train_step_mse": TrainStep(), "hier_train_step_mse": HierTrainStep(),
         "train_step_packed_mse": TrainStepPacked(), "march_train_step_mse": MarchStep(),
         "march_train_step_mse_capturable": MarchStepDeviceSizes("march_train_step_mse_capturable"),
         "march_train_step_mse_single_eval": MarchStepDeviceSizes("march_train_step_mse_single_eval"),
         "march grid_bits": MarchStepBits("march_train_step_mse_capturable"), "composite_dense": CompositeDense(),
         "composite_dense_backward": CompositeDenseBackward(), "fine_depths": FineDepths("fine_depths"),
         "fine_depths_from_tau": FineDepths("fine_depths_from_tau"), "topk_indices": Topk(), "gather_rays": GatherRays(),
         "grid_select_cells": GridSelect(), "grid_refresh": GridRefresh(), "sample_batches_dev": SampleBatches(), "encoding_grad": EncodingGrad(),
         "pack_groups": PackGroups(), "ray_entropy_packed_backward": EntropyBackward(False), "ray_entropy_dense_backward": EntropyBackward(True)}


def _bytes(t):
    return t.reshape(-1).view(U8)


def _painted(dtype, shape):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    _bytes(t).fill_(0xA5)
    return t


def _violations(dtype, shape, kinds):
    """what -> a malformed stand-in for a (dtype, shape) buffer, each a view into an allocation at least as large as the right buffer"""
    n = 1
    for s in shape:
        n *= s
    bad = {"dtype": torch.zeros(shape, dtype=SAME_SIZE[dtype], device=DEV), "short": torch.zeros(n, dtype=dtype, device=DEV)[:n - 1]}
    if n >= 2:                                                    # (a one-element tensor is contiguous whatever its stride)
        bad["strided"] = torch.zeros(2 * n, dtype=dtype, device=DEV)[::2]
    return {k: v for k, v in bad.items() if k in kinds}


@pytest.mark.parametrize("name", sorted(k for k, c in CASES.items() if c.optional))
def test_passed_buffers_are_returned_and_hold_what_an_allocating_call_returns(name):
    case = CASES[name]
    accumulates = name.startswith("ray_entropy")                   # `out` is added to: it starts at zero
    auto = case.call({})
    given = {k: torch.zeros(case.buffers[k][1], dtype=case.buffers[k][0], device=DEV) if accumulates else _painted(*case.buffers[k][:2])
             for k in case.optional}
    if case.workspace() is not None:
        given["workspace"] = _painted(U8, (int(case.workspace()),))
    res = case.call(given)
    torch.cuda.synchronize()
    for k in case.optional:
        assert res[k] is given[k], (name, k)
    spec = getattr(case, "specified", lambda r: r)
    want, got = spec(auto), spec(res)
    assert want.keys() == got.keys()
    for k in want:
        same = torch.equal(want[k], got[k]) if accumulates else torch.equal(_bytes(want[k]), _bytes(got[k]))      # (0 + -0 = +0)
        assert want[k].dtype == got[k].dtype and want[k].shape == got[k].shape and same, (name, k)
    assert "skip" not in res or float(res["skip"]) == 0.0                 # (samples were kept: pixel and grad_flat were written)


def _column_major(t):
    """The values of a 2-D tensor in column-major memory: what a data frame's columns give."""
    s = t.t().contiguous().t()
    assert not s.is_contiguous() and torch.equal(s, t)
    return s


@pytest.mark.parametrize("name,buf", [("infer", "points"), ("train_step_mse", "origins"), ("train_step_mse", "target"), ("composite_dense", "raw"),
                                      ("composite_dense", "dirs"), ("fine_depths", "u"), ("topk_indices", "keys")])
def test_a_strided_input_gives_what_the_contiguous_one_gives(name, buf):
    i, case = _inputs(), CASES[name]
    valid = {"points": i["pts"], "origins": i["o"], "target": i["tgt"], "raw": i["raw"], "dirs": i["d"], "u": i["u"], "keys": i["w"]}[buf]
    strided = _column_major(valid) if valid.dim() == 2 else torch.stack([valid, valid], 1)[:, 0]
    assert not strided.is_contiguous()
    want, got = case.call({}), case.call({buf: strided})
    torch.cuda.synchronize()
    for k in want:
        if want[k] is not None:
            assert torch.equal(_bytes(want[k]), _bytes(got[k])), (name, buf, k)


def test_sample_rays_takes_a_column_major_table():
    e, i = _eng(), _inputs()
    want = e.sample_rays(i["o"], i["d"], i["tgt"], i["w"], K, seed=3, stream_id=2)
    got = e.sample_rays(_column_major(i["o"]), _column_major(i["d"]), i["tgt"], i["w"], K, seed=3, stream_id=2)
    drawn = e.RayBatchSampler(_column_major(i["o"]), i["d"], i["tgt"], i["w"], K, seed=3, prefetch=N_BATCHES).draw(2)
    torch.cuda.synchronize()
    for a, b, c in zip(want, got, drawn):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_the_input_gradient_calls_still_take_no_grad_flat():
    i = _inputs()
    d_pts, d_o = torch.zeros(R, 3, device=DEV), torch.zeros(R, 3, device=DEV)
    i["eng"].mlp_backward_inputs(i["prep"]["f32"], i["pts"], i["tgt"], None, d_pts, "f32")
    pixel = i["eng"].render_forward(i["prep"]["f32"], i["acc"], "f32")[0]
    i["eng"].render_backward_inputs(i["prep"]["f32"], i["acc"], pixel, i["tgt"], None, d_o, None, "f32")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(d_pts).all()) and bool(torch.isfinite(d_o).all())


def test_the_refusal_table_has_every_row():
    """65 buffers, 162 malformed stand-ins (a one-element buffer has no strided view), and the 3 strided workspaces and 6 earlier families below."""
    rows = [(name, buf, what) for name in sorted(CASES) for buf, (dtype, shape, kinds) in CASES[name].buffers.items()
            for what in kinds if what != "strided" or tuple(shape) != (1,)]
    assert len({(n, b) for n, b, _ in rows}) == 65 and len(rows) == 162


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_malformed_buffer_is_refused_by_name_before_any_launch(name):
    case = CASES[name]
    for bad_name, (dtype, shape, kinds) in case.buffers.items():
        for what, bad in _violations(dtype, shape, kinds).items():
            bufs = {k: _painted(*case.buffers[k][:2]) for k in case.written if k in case.buffers}
            if "grad_flat" in case.written and "grad_flat" not in bufs:
                bufs["grad_flat"] = _painted(F32, (_inputs()["eng"].param_count,))
            before = {k: v.clone() for k, v in bufs.items() if k != bad_name}
            bufs[bad_name] = bad
            with pytest.raises(ValueError, match=rf"\b{bad_name} must "):
                case.call(bufs)
            torch.cuda.synchronize()
            for k, v in before.items():
                assert torch.equal(_bytes(bufs[k]), _bytes(v)), (name, bad_name, what, "a refused call wrote to", k)


@pytest.mark.parametrize("name", ["grid_select_cells", "grid_refresh", "sample_batches_dev"])
def test_a_workspace_goes_to_the_library_in_bytes_and_a_strided_one_is_refused(name):
    case = CASES[name]
    need = int(case.workspace())
    bufs = {k: _painted(*case.buffers[k][:2]) for k in case.written}
    before = {k: v.clone() for k, v in bufs.items()}
    with pytest.raises(ValueError, match="workspace"):
        case.call(dict(bufs, workspace=torch.empty(2 * need, dtype=U8, device=DEV)[::2]))
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(_bytes(bufs[k]), _bytes(v)), (name, "a refused call wrote to", k)
    # a float32 workspace of need / 4 (rounded up) elements holds the bytes: it is accepted, where its element count alone would be too small
    valid = {k: case.valid(k) for k in case.written}
    if name == "grid_refresh":
        valid["bits"].copy_(_inputs()["bits"])
    case.call(dict(valid, workspace=torch.empty((need + 3) // 4, dtype=F32, device=DEV)))
    torch.cuda.synchronize()


# ---- the wrappers that checked their buffers before the shared rule, in other words or another class: one buffer of each ----
def _family_calls():
    e, i = _eng(), _inputs()
    one, one64 = torch.zeros(1, device=DEV), torch.zeros(1, dtype=I64, device=DEV)
    hist = lambda dt, *s: torch.zeros(*s, dtype=dt, device=DEV)
    occs, scratch = torch.zeros(NC, device=DEV), torch.zeros(NC, device=DEV)
    return {
        "packed": ("ray_indices", I32, (R * S,), lambda t: e.composite_packed(i["pred"], t, i["pred"], i["pred"], R)),
        "visibility": ("offsets", I64, (R + 1,), lambda t: e.march_visibility(i["pred"], i["pred"], i["pred"], t, EPS, THRE)),
        "grid update": ("scratch", F32, (NC,), lambda t: e.grid_update(BOX, RES, occs, None, torch.zeros(4, device=DEV), 0.95, t)),
        "grid binarize": ("bits", I32, (WORDS,), lambda t: e.grid_binarize(BOX, RES, occs, 1e-2, hist(U8, NC), t, hist(F64, 256))),
        "round": ("counts_hist", I64, (2, 3), lambda t: e.train_round_advance(one64, torch.zeros(5, device=DEV), one, one, one, hist(I64, 3), hist(F32, 2),
                                                                              t, hist(F32, 2), one, one64)),
        "march": ("grid_bits", I32, (WORDS,), lambda t: e.march(i["o"], i["d"], BOX, NEAR, FAR, STEP, grid_bits=t, grid_aabb=BOX, grid_res=RES)),
    }


@pytest.mark.parametrize("family", ["packed", "visibility", "grid update", "grid binarize", "round", "march"])
def test_the_wrappers_that_already_checked_still_do(family):
    name, dtype, shape, call = _family_calls()[family]
    kinds = ("dtype", "strided") if family == "visibility" else ALL      # (any number of offsets is a ray count)
    for what, bad in _violations(dtype, shape, kinds).items():
        with pytest.raises(ValueError, match=rf": {name} must be "):
            call(bad)
    torch.cuda.synchronize()
