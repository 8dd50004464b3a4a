"""Full training state of the driver (nerf/run_nerf_acc.py) in one file, `trainstate.pt`, so that an interrupted run continues bit for bit.

The model file (`coarsemodel*.pth`, CPPN.save) keeps the reference's four-key dictionary and is not touched; this file sits next to it and
holds what the loop reads and the command line does not determine: parameters, BARF alpha, optimizer state (moments and `step`), the next
iteration and the learning rate, the best-PSNR / early-stop bookkeeping, the returned history, both occupancy grids (`occs`, `binary`, seed),
the device-resident state of the graph classes (render.GridTrainGraph / GridUpdateGraph / GridTrainRoundGraph), the RNG states of Python,
NumPy and torch (CPU and device), and a fingerprint of the configuration that has to match.  The workspace, the re-tiled weights and the
captured graphs are rebuilt, not saved.

Every tensor is stored on the host.  Restoring COPIES INTO the live tensors (the flat parameter buffer the Linear parameters view, Adam's
moments and step, the grids' buffers, the graphs' counters): graphs captured over them keep replaying against the same addresses.  The file
holds tensors and plain Python values only and is read with torch.load(weights_only=True).

    save_training_state(path, fingerprint=..., n_iter=..., model=..., optimizer=..., grids=[...], graphs={...}, history=[...], counters={...})
    state = load_training_state(path, fingerprint=..., model=..., optimizer=..., grids=[...], graphs={...})      # restores in place
    read_training_state(path) / restore_training_state(state, ...)                                             # the two halves of load
"""
from __future__ import annotations

import hashlib
import os
import random

import numpy as np
import torch

FORMAT_VERSION = 1
STATE_FILE = "trainstate.pt"
NONFINITE_FILE = "trainstate-before-nonfinite.pt"      # the last finite state, kept when the driver stops on a non-finite loss
STRICT = True      # restore_training_state(strict=None) reads this: a state without one of the requested pieces is an error


# ---- fingerprint --------------------------------------------------------------------------------------------------------------------------
# the driver's arguments that change the arithmetic of the run or what main() returns (n_iters, the log directory and the checkpoint flags do not)
_ARG_FIELDS = ("limited_size", "number_angles", "center_point", "binary", "sampling_strategy", "data_name", "synthetic", "img_size",
               "display_every", "sample_size", "depth_samples", "precision", "eval_precision", "march", "graph", "graph_grid_update",
               "graph_rounds", "single_eval", "adam", "host_sampler", "seed", "out_bias_init", "barf_start", "barf_stop")


def _plain(v):
    if isinstance(v, (bool, int, float, str)) or v is None:
        return v
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return str(v)


def ray_table_checksum(ray_table) -> str:
    """sha256 over the bytes of the training ray table (origins, directions, pixels, weights), as float32 on the host."""
    h = hashlib.sha256()
    for t in ray_table:
        h.update(np.ascontiguousarray(torch.as_tensor(t).detach().to("cpu", torch.float32).numpy()).tobytes())
    return h.hexdigest()


def config_fingerprint(args, model_definition: dict, ray_table) -> dict:
    """The configuration a state file belongs to: `args` (the driver's namespace), the model definition (its `device` left out) and the
    training ray table (row count and checksum).  A flat dict of plain values; field names are what a mismatch reports."""
    fp = {name: _plain(getattr(args, name, None)) for name in _ARG_FIELDS}
    if getattr(args, "entropy_weight", 0.0):      # (present only when the term is on: state files written without the flag keep their fingerprint)
        fp["entropy_weight"] = float(args.entropy_weight)
    if getattr(args, "grid_init", None):          # (likewise: --grid_init hull and its three parameters are named only when set)
        fp["grid_init"] = str(args.grid_init)
        for name in ("hull_margin", "hull_max_rejects", "hull_threshold"):
            fp[name] = _plain(getattr(args, name, None))
    for k, v in sorted(model_definition.items()):
        if k != "device":
            fp[f"model.{k}"] = _plain(v)
    fp["n_rays"] = int(torch.as_tensor(ray_table[0]).shape[0])
    fp["ray_table_sha256"] = ray_table_checksum(ray_table)
    return fp


def compare_fingerprints(saved: dict, current: dict):
    """ValueError naming every field that differs."""
    diff = [k for k in sorted(set(saved) | set(current)) if saved.get(k, "<absent>") != current.get(k, "<absent>")]
    if diff:
        raise ValueError("resume: the state file belongs to a different configuration; differing fields: " + ", ".join(
            f"{k} (saved {saved.get(k, '<absent>')!r}, now {current.get(k, '<absent>')!r})" for k in diff))


# ---- RNG ----------------------------------------------------------------------------------------------------------------------------------
def rng_state() -> dict:
    """Python, NumPy and torch (CPU, and the current device) generator states as tensors and plain values."""
    kind, keys, pos, has_gauss, gauss = np.random.get_state()
    version, words, gauss_next = random.getstate()
    st = dict(numpy=dict(kind=str(kind), keys=torch.from_numpy(np.asarray(keys, dtype=np.uint32).astype(np.int64)), pos=int(pos),
                         has_gauss=int(has_gauss), gauss=float(gauss)),
              python=dict(version=int(version), words=list(words), gauss_next=gauss_next),
              torch_cpu=torch.get_rng_state().clone())
    if torch.cuda.is_available():
        st["torch_device"] = torch.cuda.get_rng_state().clone()      # the current device's: the driver runs on one
    return st


def set_rng_state(st: dict):
    n = st["numpy"]
    np.random.set_state((n["kind"], n["keys"].numpy().astype(np.uint32), n["pos"], n["has_gauss"], n["gauss"]))
    p = st["python"]
    random.setstate((p["version"], tuple(p["words"]), p["gauss_next"]))
    torch.set_rng_state(st["torch_cpu"])
    if "torch_device" in st and torch.cuda.is_available():
        torch.cuda.set_rng_state(st["torch_device"])


# ---- pieces -------------------------------------------------------------------------------------------------------------------------------
def _to_host(v):
    if torch.is_tensor(v):
        return v.detach().to("cpu", copy=True)
    if isinstance(v, dict):
        return {k: _to_host(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return type(v)(_to_host(x) for x in v)
    return v


def optimizer_state(optimizer) -> dict:
    """optimizer.state_dict() with every tensor on the host (a tensor learning rate included)."""
    return _to_host(optimizer.state_dict())


def load_optimizer_state(optimizer, sd: dict):
    """optimizer.load_state_dict without rebinding: where the optimizer already holds state (the graph classes create it before they
    capture), the saved moments and `step` are copied into the live tensors, and a tensor learning rate is filled in place.  State that
    does not exist yet is created as torch does (moments on the parameter's device; `step` there too for the fused / capturable Adam)."""
    groups, saved_groups = optimizer.param_groups, sd["param_groups"]
    if len(groups) != len(saved_groups) or any(len(g["params"]) != len(s["params"]) for g, s in zip(groups, saved_groups)):
        raise ValueError("resume: the optimizer's parameter groups differ from the saved ones")
    with torch.no_grad():
        for g, s in zip(groups, saved_groups):
            for k, v in s.items():
                if k == "params":
                    continue
                live = g.get(k)
                if torch.is_tensor(live):      # (captured by address: --graph keeps the learning rate in a device tensor)
                    live.copy_(torch.as_tensor(v))
                else:
                    g[k] = v.item() if torch.is_tensor(v) and v.numel() == 1 else v
            on_device_step = bool(g.get("fused") or g.get("capturable"))
            for p, idx in zip(g["params"], s["params"]):
                saved = sd["state"].get(idx)
                if saved is None:
                    continue
                live = optimizer.state[p] if p in optimizer.state else None
                if not live:
                    live = optimizer.state[p]
                    for k, v in saved.items():
                        if not torch.is_tensor(v):
                            live[k] = v
                        elif k == "step":
                            live[k] = v.to(p.device if on_device_step else "cpu", copy=True)
                        else:
                            live[k] = v.to(p.device, copy=True)
                    continue
                for k, v in saved.items():
                    if torch.is_tensor(live.get(k)):
                        live[k].copy_(v)
                    else:
                        live[k] = v


def model_state(model) -> dict:
    st = dict(state_dict=_to_host(model.state_dict()))
    if getattr(model, "use_pos_enc", None) == "barf":
        st["barf_alpha"] = float(model.barf_alpha)
    return st


def load_model_state(model, st: dict):
    """Parameters copied into the live ones (load_state_dict copies; the Linear parameters stay views of the flat buffer), the BARF
    schedule put back, the cached re-tiled weights marked stale (their buffers stay: captured graphs re-tile into them)."""
    with torch.no_grad():
        model.load_state_dict(st["state_dict"])
    if "barf_alpha" in st and hasattr(model, "update_barf_alpha"):
        model.update_barf_alpha(st["barf_alpha"], "pts")
    if hasattr(model, "mark_prepared_stale"):
        model.mark_prepared_stale()


# ---- the file -----------------------------------------------------------------------------------------------------------------------------
def state_path(path: str) -> str:
    """A state file, or the `trainstate.pt` inside a directory."""
    return os.path.join(path, STATE_FILE) if os.path.isdir(path) else path


def save_training_state(path, *, fingerprint: dict, n_iter: int, model=None, optimizer=None, grids=(), graphs=None, history=(),
                        counters=None, rng: bool = True) -> str:
    """Write the state after iteration n_iter - 1 (`n_iter` = the next iteration to run) atomically: to a temporary name in the same
    directory, flushed, then os.replace.  A save that fails half-way leaves the previous file as it was.
    grids: OccupancyGrids (training_state()); graphs: {name: object with state_dict()}; counters: plain values and tensors."""
    state = dict(format_version=FORMAT_VERSION, fingerprint=dict(fingerprint), n_iter=int(n_iter), history=_to_host(list(history)),
                 counters=_to_host(dict(counters or {})))
    if model is not None:
        state["model"] = model_state(model)
    if optimizer is not None:
        state["optimizer"] = optimizer_state(optimizer)
    if grids:
        state["grids"] = [_to_host(g.training_state()) for g in grids]
    if graphs:
        state["graphs"] = {name: _to_host(g.state_dict()) for name, g in graphs.items()}
    if rng:
        state["rng"] = rng_state()
    path = str(path)
    tmp = f"{path}.tmp.{os.getpid()}"
    try:
        with open(tmp, "wb") as f:
            torch.save(state, f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    return path


def read_training_state(path) -> dict:
    """The state dict of a file (or of the trainstate.pt in a directory), tensors on the host.  A newer format version is refused."""
    state = torch.load(state_path(str(path)), map_location="cpu", weights_only=True)
    version = state.get("format_version") if isinstance(state, dict) else None
    if not isinstance(version, int):
        raise ValueError(f"resume: {path} is not a training-state file")
    if version > FORMAT_VERSION:
        raise ValueError(f"resume: {path} has format version {version}; this code reads up to {FORMAT_VERSION}")
    return state


def restore_training_state(state: dict, *, fingerprint=None, model=None, optimizer=None, grids=(), graphs=None, rng: bool = True,
                           strict=None) -> dict:
    """Check the fingerprint, then restore every object passed, in place.  strict (default: the module's STRICT): a requested piece that
    the state lacks is a ValueError; strict=False skips it.  Returns `state` (n_iter, history, counters are the caller's to apply)."""
    strict = STRICT if strict is None else strict
    if fingerprint is not None:
        compare_fingerprints(state["fingerprint"], fingerprint)

    def piece(name, wanted):
        if not wanted:
            return None
        if name not in state:
            if strict:
                raise ValueError(f"resume: the state file holds no '{name}'")
            return None
        return state[name]

    st = piece("model", model is not None)
    if st is not None:
        load_model_state(model, st)
    st = piece("optimizer", optimizer is not None)
    if st is not None:
        load_optimizer_state(optimizer, st)
    st = piece("grids", bool(grids))
    if st is not None:
        if len(st) != len(grids):
            raise ValueError(f"resume: {len(st)} occupancy grids saved, {len(grids)} to restore")
        for g, s in zip(grids, st):
            g.load_training_state(s)
    st = piece("graphs", bool(graphs))
    if st is not None:
        if set(st) != set(graphs):
            raise ValueError(f"resume: graph state saved for {sorted(st)}, to restore: {sorted(graphs)}")
        for name, g in graphs.items():
            g.load_state_dict(st[name])
    st = piece("rng", rng)
    if st is not None:
        set_rng_state(st)
    return state


def load_training_state(path, **kwargs) -> dict:
    """read_training_state + restore_training_state."""
    return restore_training_state(read_training_state(path), **kwargs)
