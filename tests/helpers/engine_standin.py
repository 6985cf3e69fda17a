"""A HipEngine whose library is a stand-in, so that every method runs on CPU tensors and what it hands to the C ABI can be written down
(tests/test_engine_calls_cpu.py, tests/helpers/engine_cases.py).

StandinLib answers every name of _lib.SIGNATURES: it asserts the argument count, passes each argument that is not None through its
argtype's from_param (the conversion ctypes itself would make) and returns fixed small values.  standin() patches what a method needs
outside the library: torch.cuda (availability, the current stream), pin_memory (which also collects the uploaded tables), _lib.load and
the engine's _p, whose pointers then carry the tensor they came from, so that a line names what was pointed at, not an address."""
import contextlib
import ctypes as C
import sys
import types
from unittest import mock

import numpy as np
import torch

from smalltts_amd import _lib

HANDLE, STREAM = 0x5150, 0x57          # what smtts_create hands out, the current stream's handle
BYTES, HOP = 256, 8                    # every *_bytes query, smtts_codec_hop
STAGE_T, STAGE_C = 3, 5                # t_out / c_out of smtts_test_codec_stage
QUERIES = ("smtts_codec_hop", "smtts_has_part", "smtts_last_error")   # with *_bytes: the calls a refused method may make


class Ptr(C.c_void_p):
    """What _p returns under the stand-in: the address, and the tensor itself (kept alive; named once the method has returned)."""


def ptr(t):
    if t is None:
        return None
    p = Ptr(t.data_ptr())
    p.tensor = t
    return p


class StandinLib:
    def __init__(self, zero=(), fail=(), parts=1, saturated=()):
        self.zero, self.fail, self.parts, self.saturated = set(zero), set(fail), parts, tuple(saturated)
        self.calls = []      # (name, [argument as recorded: str or Ptr])
        self.error = None    # what the method raised

    def __getattr__(self, name):
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        res, argtypes = _lib.SIGNATURES[name]
        assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for {len(argtypes)} parameters"
        for a, ty in zip(args, argtypes):
            if a is not None:
                ty.from_param(a)
        self.calls.append((name, [self._note(name, i, a, ty, args) for i, (a, ty) in enumerate(zip(args, argtypes))]))
        return self._answer(name, args, res)

    @staticmethod
    def _note(name, i, a, ty, args):
        if a is None:
            return "null"
        if isinstance(a, Ptr):
            return a
        if ty is C.c_void_p:
            v = a.value if isinstance(a, C.c_void_p) else int(a)
            if name in ("smtts_sample_align", "smtts_sample_pinned") and i == 24:    # the step flags: num_steps bytes on the host
                return "flags:" + C.string_at(v, int(args[3])).hex()
            return {HANDLE: "h", STREAM: "stream"}.get(v, "host")
        if type(a).__name__ == "CArgObject":
            return "&" + type(a._obj).__name__
        if isinstance(a, C.Array):
            return f"char[{len(a)}]" if a._type_ is C.c_char else "[" + ",".join(str(v) for v in a) + "]"
        if isinstance(a, C._SimpleCData):
            a = a.value
        if isinstance(a, bytes):
            return a.decode()
        return repr(float(a)) if ty is C.c_float else str(int(a))

    def _answer(self, name, args, res):
        if name == "smtts_test_scorer_tap_bytes":       # every slot as large as its buffer, rounded up to 256 bytes
            from smalltts_amd.engine_hooks import scorer_tap_shapes
            at = 0
            for i, sh in enumerate(scorer_tap_shapes({0: "asr", 1: "sv"}[int(args[1])], int(args[2]), int(args[3])).values()):
                args[4][i] = at
                at += (4 * int(np.prod(sh)) + 255) // 256 * 256
            return at
        if name.endswith("_bytes"):
            return 0 if name in self.zero else BYTES
        if name == "smtts_codec_hop":
            return HOP
        if name == "smtts_has_part":
            return self.parts
        if name in ("smtts_last_error", "smtts_range_report", "smtts_version"):
            return b"stand-in text"
        if name == "smtts_alpha_sigma":
            args[1]._obj.value, args[2]._obj.value = 0.5, 0.25
            return None
        if name in self.fail:
            return 1
        if name == "smtts_create":
            args[1]._obj.value = HANDLE
        if name == "smtts_test_codec_stage":
            args[10]._obj.value, args[11]._obj.value = STAGE_T, STAGE_C
        if name == "smtts_profile_report":
            args[1].value = b'{"kernels": []}'
        if name in ("smtts_get_saturations", "smtts_peek_saturations"):
            for i in self.saturated:
                args[1][i] = 1
        return 0


@contextlib.contextmanager
def standin(lib, uploads):
    """The patches under which HipEngine() and its methods run on the CPU against `lib`; pinned tables are appended to `uploads`."""
    mods = [m for m in (sys.modules.get("smalltts_amd.engine"), sys.modules.get("smalltts_amd.engine_hooks")) if m is not None]

    def pin(t):
        uploads.append(t)
        return t

    with contextlib.ExitStack() as st:
        st.enter_context(mock.patch.object(torch.cuda, "is_available", lambda: True))
        st.enter_context(mock.patch.object(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=STREAM)))
        st.enter_context(mock.patch.object(torch.Tensor, "pin_memory", pin))
        st.enter_context(mock.patch.object(_lib, "load", lambda: lib))
        for m in mods:
            if hasattr(m, "_p"):
                st.enter_context(mock.patch.object(m, "_p", ptr))
        yield


def make_engine(lib):
    """HipEngine() through its own __init__ (inside standin()), then moved to the CPU; the calls of the construction are dropped."""
    from smalltts_amd.engine import HipEngine
    eng = HipEngine(0)
    eng.device = torch.device("cpu")
    del lib.calls[:]
    return eng


# ---- writing a call down -----------------------------------------------------------------------------------------------------------
def _named(prefix, v, out):
    if isinstance(v, torch.Tensor):
        out.append((prefix, v))
    elif isinstance(v, dict):
        for k, x in v.items():
            _named(f"{prefix}.{k}", x, out)
    elif isinstance(v, (list, tuple)):
        for i, x in enumerate(v):
            _named(f"{prefix}[{i}]", x, out)
    elif isinstance(v, types.SimpleNamespace):
        for k, x in vars(v).items():
            _named(f"{prefix}.{k}" if prefix else k, x, out)


def _label(t, known):
    """`t` as base + byte offset: the known tensor that starts where t starts, else the first one that shares its storage."""
    def same(k):
        return k.device == t.device and k.untyped_storage().data_ptr() == t.untyped_storage().data_ptr()
    for name, k in known:
        if same(k) and k.data_ptr() == t.data_ptr():
            return f"{name}+0"
    for name, k in known:
        if same(k):
            return f"{name}+{t.data_ptr() - k.data_ptr()}"
    return f"tmp:{str(t.dtype)[6:]}{tuple(t.shape)}"


def _show(v, operands):
    if isinstance(v, torch.Tensor):
        for name, k in operands:
            if k is v:
                return f"={name}"
        return f"{str(v.dtype)[6:]}{tuple(v.shape)}"
    if isinstance(v, np.ndarray):
        return f"ndarray:{v.dtype}{v.shape}"
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}: {_show(x, operands)}" for k, x in v.items()) + "}"
    if isinstance(v, (list, tuple)):
        return "(" + ", ".join(_show(x, operands) for x in v) + ")"
    return repr(v)


def record(title, fn, operands, *, env_engine=None, **lib_opts):
    """One section: `fn(eng, operands)` on a fresh stand-in engine (or on what env_engine(lib) builds inside the patches).
    -> (lines, lib): the header, one line per C call, one per uploaded table, then '-> result' or '!! Exception: text'."""
    lib, uploads = StandinLib(**lib_opts), []
    lines = [f"== {title}"]
    eng = ret = err = None
    with standin(lib, uploads):
        try:
            eng = (env_engine or make_engine)(lib)
            ret = fn(eng, operands)
        except (ValueError, RuntimeError) as e:
            err = lib.error = e
    ops = []
    _named("", operands, ops)
    known = list(ops)
    _named("ret", ret, known)
    ws = [("ws", w) for w in ([getattr(eng, "_ws", None)] if eng is not None else []) if w is not None]
    known += ws + [(f"table{i}", t) for i, t in enumerate(uploads)]
    for name, args in lib.calls:
        lines.append(name + " " + " ".join(_label(a.tensor, known) if isinstance(a, Ptr) else a for a in args))
    addr = {k.data_ptr(): name for name, k in ops if k.device.type == "cpu" and k.numel()}
    for i, t in enumerate(uploads):
        def val(v):
            return f"&{addr[v]}" if v in addr else str(v)
        rows = t.tolist()
        body = ("[" + ", ".join("[" + ", ".join(val(v) for v in r) + "]" for r in rows) + "]" if t.dim() == 2
                else "[" + ", ".join(val(v) for v in rows) + "]")
        lines.append(f"table{i} {str(t.dtype)[6:]}{tuple(t.shape)} {body}")
    lines.append(f"!! {type(err).__name__}: {err}" if err is not None else f"-> {_show(ret, ops)}")
    return lines, lib
