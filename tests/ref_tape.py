"""The compiled reference (oracle/_ref, built by `make -C oracle ref` only where the reference's sources are at hand) on tape.

Tests marked `ref` hold the oracle and the host driver to the reference's own results. They reach the reference through the `ref`
fixture, a RefTape: the surface of oracle/ref_py.py the tests use, every call of it recorded once against the live library and
replayed everywhere else from tests/golden/ref_tapes/<test module>.npz -- the test sees the very values the reference returned
for the very same arguments, and a call whose arguments differ from the recorded one fails the test.

  MSC_REF_TAPE unset     replay the tape (no reference needed)
  MSC_REF_TAPE=live      call the compiled reference, no tape
  MSC_REF_TAPE=record    call the compiled reference and (re)write the test's tape:  MSC_REF_TAPE=record python -m pytest tests -m ref
"""
import base64
import ctypes as C
import hashlib
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPES = os.path.join(ROOT, "tests", "golden", "ref_tapes")
MODES = ("replay", "live", "record")


def mode():
    m = os.environ.get("MSC_REF_TAPE", "") or "replay"
    if m not in MODES:
        raise ValueError("MSC_REF_TAPE=%s: one of %s" % (m, ", ".join(MODES[1:])))
    return m


class _Obj:
    """a reference object (Point, Model, or what a test wraps with RefTape.new): attribute access = a method call on tape"""

    def __init__(self, tape, kind, oid, live):
        self._tape, self._kind, self._id, self._live = tape, kind, oid, live

    def __getattr__(self, attr):
        if attr.startswith("_"):
            raise AttributeError(attr)
        name = self._kind + "." + attr

        def method(*args):
            if name in self._tape.NEW:
                return self._tape._new(self._kind, name, args, lambda: getattr(self._live, attr)(*_live(args)))
            return self._tape._call(name, args, lambda: getattr(self._live, attr)(*_live(args)))
        return method


def _live(x):
    if isinstance(x, _Obj):
        return x._live
    if isinstance(x, (list, tuple)):
        return type(x)(_live(v) for v in x)
    return x


def _digest(h, x):
    """the arguments of a call, canonically: objects by their tape id, repository paths relative to the repository"""
    if isinstance(x, _Obj):
        h.update(b"O%d;" % x._id)
    elif x is None:
        h.update(b"N;")
    elif isinstance(x, (bool, np.bool_)):
        h.update(b"T;" if x else b"F;")
    elif isinstance(x, (int, np.integer)):
        h.update(b"I%d;" % int(x))
    elif isinstance(x, (float, np.floating)):
        h.update(b"D" + repr(float(x)).encode() + b";")
    elif isinstance(x, bytes):
        h.update(b"B%d:" % len(x) + x)
    elif isinstance(x, str):
        if os.path.isabs(x) and x.startswith(ROOT + os.sep):
            x = os.path.relpath(x, ROOT)
        s = x.encode()
        h.update(b"S%d:" % len(s) + s)
    elif isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        h.update(b"A" + a.dtype.str.encode() + repr(a.shape).encode() + a.tobytes())
    elif isinstance(x, (list, tuple)):
        h.update(b"L%d(" % len(x))
        for v in x:
            _digest(h, v)
        h.update(b")")
    else:
        raise TypeError("cannot put a %s on tape" % type(x).__name__)


def _key(name, args):
    h = hashlib.sha1()
    _digest(h, list(args))
    return name + ":" + h.hexdigest()[:8]


def _enc(x, arrays):
    if isinstance(x, C.Array):
        x = np.array(x)
    if isinstance(x, np.ndarray):
        arrays.append(np.ascontiguousarray(x))
        return {"a": len(arrays) - 1}
    if isinstance(x, (np.bool_, np.integer, np.floating)):
        return x.item()
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, bytes):
        return {"b": base64.b64encode(x).decode()}
    if isinstance(x, tuple):
        return {"t": [_enc(v, arrays) for v in x]}
    if isinstance(x, list):
        return [_enc(v, arrays) for v in x]
    if isinstance(x, dict):
        return {"d": {k: _enc(v, arrays) for k, v in x.items()}}
    raise TypeError("cannot put a %s on tape" % type(x).__name__)


def _dec(x, arrays):
    if isinstance(x, list):
        return [_dec(v, arrays) for v in x]
    if isinstance(x, dict):
        if "a" in x:
            return arrays[x["a"]].copy()
        if "b" in x:
            return base64.b64decode(x["b"])
        if "t" in x:
            return tuple(_dec(v, arrays) for v in x["t"])
        return {k: _dec(v, arrays) for k, v in x["d"].items()}
    return x


class RefTape:
    """ref_py's surface as the tests use it, on tape. One per test (`name` = the test's node name)."""
    NEW = {"Point", "Model", "Point.clone"}          # calls that hand back a reference object
    RAISES = (ValueError, RuntimeError)              # what the reference may answer with instead of a value

    def __init__(self, module, name):
        self.mode = mode()
        self.path = os.path.join(TAPES, module + ".npz")
        self.name = name
        self.n_obj = 0
        self.keys, self.outs, self.arrays = [], [], []
        self.pos = 0
        if self.mode == "replay":
            if not os.path.exists(self.path):
                raise FileNotFoundError("%s: no tape (MSC_REF_TAPE=record where oracle/_ref is built writes it)" % os.path.relpath(self.path, ROOT))
            with np.load(self.path, allow_pickle=False) as z:
                if name + ".json" not in z.files:
                    raise KeyError("%s holds no tape of %s (MSC_REF_TAPE=record where oracle/_ref is built writes it)" % (os.path.relpath(self.path, ROOT), name))
                rec = json.loads(str(z[name + ".json"]))
                self.arrays = [z["%s.%d" % (name, i)] for i in range(rec["n_arrays"])]
            self.keys, self.outs = rec["keys"], rec["outs"]
            self.ref = None
        else:
            from oracle import ref_py
            if not ref_py.available():
                raise RuntimeError("MSC_REF_TAPE=%s: oracle/_ref/libmsc_ref.so is not built (needs the reference's sources at build time)" % self.mode)
            ref_py.lib()
            self.ref = ref_py

    # -- the two primitives: a call that returns a value, a call that returns a reference object

    def _call(self, name, args, live):
        key = _key(name, args)
        if self.mode == "replay":
            if self.pos >= len(self.keys):
                raise AssertionError("%s: call %d (%s) to the reference is not on the tape" % (self.name, self.pos, name))
            if self.keys[self.pos] != key:
                raise AssertionError("%s: call %d to the reference is %s, the tape holds %s (the test took another path than when it was "
                                     "recorded)" % (self.name, self.pos, key, self.keys[self.pos]))
            out = self.outs[self.pos]
            self.pos += 1
            if isinstance(out, dict) and "raise" in out:
                raise {c.__name__: c for c in self.RAISES}[out["raise"]](out["message"])
            return _dec(out, self.arrays)
        try:
            value = live()
        except self.RAISES as e:
            if self.mode == "record":
                self.keys.append(key)
                self.outs.append({"raise": type(e).__name__, "message": str(e)})
            raise
        if self.mode == "record":
            self.keys.append(key)
            self.outs.append(_enc(value, self.arrays))
            value = _dec(self.outs[-1], self.arrays)          # the test sees what a replay will see
        return value

    def _new(self, kind, name, args, live):
        made = []
        self._call(name, args, lambda: made.append(live()))          # on tape: None, or the exception the reference threw
        oid = self.n_obj
        self.n_obj += 1
        return _Obj(self, kind, oid, made[0] if made else None)

    def close(self, passed):
        """record: write this test's tape into its module's file; replay: every recorded call was made"""
        if self.mode == "record" and passed:
            os.makedirs(TAPES, exist_ok=True)
            entries = {}
            if os.path.exists(self.path):
                with np.load(self.path, allow_pickle=False) as z:
                    entries = {k: z[k] for k in z.files if k != self.name + ".json" and not k.startswith(self.name + ".")}
            entries[self.name + ".json"] = np.array(json.dumps({"keys": self.keys, "outs": self.outs, "n_arrays": len(self.arrays)}))
            for i, a in enumerate(self.arrays):
                entries["%s.%d" % (self.name, i)] = a
            np.savez_compressed(self.path, **entries)
        if self.mode == "replay" and passed:
            assert self.pos == len(self.keys), "%s: %d of %d recorded calls to the reference were not made" % (self.name, len(self.keys) - self.pos, len(self.keys))

    # -- oracle/ref_py.py's surface

    def Point(self, dtype, seq, k, strip=False):
        return self._new("Point", "Point", (dtype, seq, k, strip), lambda: self.ref.Point(dtype, seq, k, strip=strip))

    def Model(self, dtype, path):
        return self._new("Model", "Model", (dtype, path), lambda: self.ref.Model(dtype, path))

    def encode(self, seq):
        return self._call("encode", (seq,), lambda: self.ref.encode(seq))

    def raw_feature(self, flag, a, b):
        return self._call("raw_feature", (flag, a, b), lambda: self.ref.raw_feature(flag, a._live, b._live))

    def mean_nearest(self, pts):
        return self._call("mean_nearest", (pts,), lambda: self.ref.mean_nearest(_live(pts)))

    def train_class(self, *args):
        return self._call("train_class", args, lambda: self.ref.train_class(*_live(args)))

    def set_threads(self, n):
        return self._call("set_threads", (n,), lambda: self.ref.lib().ref_set_threads(n))

    # -- anything else a test reaches through the library: `factory()` / `fn(*args)` run only against the live reference

    def new(self, kind, factory, *args):
        """a test's own wrapper of the library (kind names it on tape; args = what the wrapper is built from)"""
        return self._new(kind, kind, args, factory)

    def call(self, name, fn, *args):
        return self._call(name, args, lambda: fn(*args))

    def lib(self):
        return self.ref.lib()
