"""Reading the reference's ``last.ckpt`` into the model a run builds (``REFace/scripts/VFace_inference_batch.py:118-135``)."""
from __future__ import annotations

import torch


class _StubUnpickler:
    """``pickle_module`` for ``torch.load`` of a checkpoint written by the reference's pytorch_lightning==1.4.2
    (``REFace/environment.yml``): its ``callbacks`` / ``hyper_parameters`` entries pickle CLASS objects (the ModelCheckpoint
    class as a dict key) and omegaconf containers, which ``weights_only=True`` rejects and which are not importable here.

    ``find_class`` resolves EXACTLY the (module, name) pairs of torch's own ``weights_only`` allow-list
    (``torch._weights_only_unpickler._get_allowed_globals``: the ``_rebuild_*`` helpers, storages, dtypes, ``torch.Size``,
    ``collections.OrderedDict`` ..) plus the numpy scalar / dtype reconstructors -- never a whole package: every other global,
    including every other ``torch.*`` / ``numpy.*`` / ``builtins`` name (``torch.utils.collect_env.run``, ``torch.hub.load``,
    ``numpy.load``, ``os.system`` ..), becomes an inert placeholder class whose construction, call and ``__setstate__`` do
    nothing.  No callable outside the allow-list is ever invoked (``tests/test_host_cpu.py`` feeds it hostile pickles).
    It is used only when the caller asks for it (``load_checkpoint(.., stub_unknown_globals=True)`` /
    ``--ckpt_stub_unknown_globals``), never as a silent fallback."""
    import pickle as _pickle

    _NUMPY_OK = frozenset({("numpy.core.multiarray", "scalar"), ("numpy._core.multiarray", "scalar"),
                           ("numpy", "dtype"), ("numpy.core.multiarray", "_reconstruct"),
                           ("numpy._core.multiarray", "_reconstruct"), ("numpy", "ndarray")})
    _allowed = None

    @classmethod
    def allowed(cls) -> dict:
        if cls._allowed is None:
            from torch._weights_only_unpickler import _get_allowed_globals
            cls._allowed = dict(_get_allowed_globals())
        return cls._allowed

    class Unpickler(_pickle.Unpickler):
        _stubs: dict = {}

        def find_class(self, module, name):
            hit = _StubUnpickler.allowed().get(f"{module}.{name}")
            if hit is not None:
                return hit
            if (module, name) in _StubUnpickler._NUMPY_OK:
                return super().find_class(module, name)
            key = (module, name)
            if key not in self._stubs:
                def _new(cls, *a, **k):
                    return object.__new__(cls)
                self._stubs[key] = type(name, (), {"__module__": module, "__new__": _new, "__init__": lambda self, *a, **k: None,
                                                   "__setstate__": lambda self, st: None, "__call__": lambda self, *a, **k: None,
                                                   "append": lambda self, *a: None, "extend": lambda self, *a: None,
                                                   "__setitem__": lambda self, *a: None})
            return self._stubs[key]

    @staticmethod
    def load(f, **kw):
        return _StubUnpickler.Unpickler(f, **kw).load()

    @staticmethod
    def loads(b, **kw):
        import io
        return _StubUnpickler.Unpickler(io.BytesIO(b), **kw).load()

    __name__ = "vface_stub_pickle"


def load_checkpoint(model, path: str, with_vae: bool = False, stub_unknown_globals: bool = False) -> str:
    """Load ``last.ckpt`` of the reference (``VFace_inference_batch.py:118-135``: ``torch.load`` -> ``["state_dict"]`` ->
    ``load_state_dict(strict=False)``) into ``model``.  Only the keys of what this build runs are taken:
    ``model.diffusion_model.*`` always, ``first_stage_model.*`` when the first stage was built (``with_vae``),
    ``cond_stage_model.*`` and the projections of ``conditioning_with_feat`` when the conditioning stage was built (the text tower
    and the other entries FrozenCLIPEmbedder holds without reading are dropped); the ArcFace weights of a full LDM checkpoint
    (``face_ID_model.facenet.*``) when the identity network was built (``--arcface``), otherwise they are outside the path and ignored.  Unlike the reference's
    non-strict load, a checkpoint that does not cover every parameter of the path raises instead of silently running on
    default-initialised weights.

    The load is ``weights_only=True``.  A pytorch_lightning checkpoint carries class-keyed callback state that the safe loader
    rejects: pass ``stub_unknown_globals=True`` (``--ckpt_stub_unknown_globals``) to read it through ``_StubUnpickler`` (exact
    allow-list, inert placeholders for everything else).  There is no automatic fallback: a file that fails the safe loader
    raises, naming the flag."""
    import pickle
    if stub_unknown_globals:
        ck = torch.load(path, map_location="cpu", weights_only=False, pickle_module=_StubUnpickler)
    else:
        try:
            ck = torch.load(path, map_location="cpu", weights_only=True)
        except pickle.UnpicklingError as e:
            raise RuntimeError(
                f"{path}: the weights-only loader rejected this checkpoint ({str(e).splitlines()[0][:200]}).  If it is a "
                "pytorch_lightning checkpoint (callbacks / hyper_parameters pickle class objects), pass "
                "--ckpt_stub_unknown_globals (load_checkpoint(.., stub_unknown_globals=True)): tensors load through torch's own "
                "allow-list and every other global becomes an inert placeholder") from e
    sd = ck.get("state_dict", ck) if isinstance(ck, dict) else ck
    prefixes = ("model.diffusion_model.",) + (("first_stage_model.",) if with_vae else ())
    if hasattr(model, "cond_stage_model"):      # the conditioning stage was built: its encoder and the four projections load too
        prefixes += ("cond_stage_model.", "proj_out_source.", "proj_out_target.", "ID_proj_out.", "landmark_proj_out.", "learnable_vector")
    if hasattr(model, "face_ID_model"):
        prefixes += ("face_ID_model.facenet.",)
    taken = {k: v for k, v in sd.items() if k.startswith(prefixes) and torch.is_tensor(v)}
    if not taken:
        raise RuntimeError(f"{path}: no key starts with {prefixes} -- not an LDM checkpoint of this model "
                           f"(first keys: {list(sd)[:5]})")
    missing, unexpected = model.load_state_dict(taken, strict=False)
    hot = [k for k in missing if k.startswith(prefixes)]
    if hot or unexpected:
        raise RuntimeError(f"{path}: {len(hot)} parameter(s) of the denoising path missing (first: {hot[:5]}), "
                           f"{len(unexpected)} unexpected key(s) (first: {list(unexpected)[:5]})")
    return (f"loaded {path}: {len(taken)} tensors under {', '.join(prefixes)} matched every parameter of the path "
            f"({len(sd) - len(taken)} checkpoint entries outside it ignored)")
