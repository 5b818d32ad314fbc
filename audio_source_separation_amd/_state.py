"""Public attributes that live in HBM and materialise as NumPy arrays on demand.

The reference keeps `demix_filter`, `basis`, `activation`, `estimation` as NumPy attributes that
callbacks read after every iteration (egs/bss-example/ilrma/test_gauss-ilrma.ipynb cells 69-78)
and that `_reset` warm-starts from via `hasattr` (src/bss/ilrma.py:67-72, 88-104).  Here the
authoritative copy is a device tensor; the NumPy view is downloaded lazily and cached until a
kernel touches the tensor again, so a loop without callbacks never leaves the GPU.  The downloaded view is a tracked
ndarray (round 4): an in-place edit -- `model.basis[...] *= s`, `model.demix_filter[f] = w`, also through slices of it --
marks the device copy stale, and the next kernel uploads the edited host array first, as in the reference, whose
attributes are plain NumPy arrays (src/bss/ilrma.py:97-104).  Edits of an OLD snapshot (the model has been updated
since it was handed out) do nothing, like edits of any copy.
"""
import numpy as np

from . import _lib
from ._device import to_device, to_numpy, torch
from ._loss import LazyLossList


class _Entry:
    __slots__ = ("host", "dev", "owner", "sig")

    def __init__(self, host=None, dev=None, owner=None):
        self.host = host
        self.dev = dev
        self.owner = owner  # the model: an edit of state invalidates a loss value parked for the next pass
        self.sig = None  # _signature(host) when host and dev were last known to agree


_SIG_COLS = 1024
_GOLD = np.uint64(0x9E3779B97F4A7C15)


def _sig_weights(n, salt):
    """n odd 64-bit multipliers (a fixed sequence: Weyl steps of the golden ratio, forced odd)."""
    with np.errstate(over="ignore"):
        return (np.arange(1 + salt, n + 1 + salt, dtype=np.uint64) * _GOLD) | np.uint64(1)


def _signature(a):
    """Cheap POSITION-DEPENDENT content signature of a host array (two reductions over its 64-bit words laid out as rows
    of 1024: the row sums and the column sums, each combined with a fixed sequence of odd multipliers modulo 2^64; ~0.2 ms
    per MB).  TrackedArray sees writes made THROUGH it; a write through a plain view of the same memory (np.asarray(a),
    a.view(np.ndarray), torch.from_numpy(a)) or into an array the caller assigned and kept does not pass any hook -- the
    signature taken when host and device agreed is compared before the device copy is reused (DeviceState._dev), so such
    an edit still reaches the next kernel, as it would in the reference (plain NumPy attributes, src/bss/ilrma.py:97-104).
    Round 5's signature (plain sum + xor of the words) was blind to every reordering -- swapping two source rows of the
    demixing filter, flipping an array in place -- because both reductions are permutation-invariant; here a word that
    moves changes its row weight, its column weight or both."""
    try:
        b = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        n8 = b.size // 8
        w = b[:n8 * 8].view(np.uint64)
        rows = n8 // _SIG_COLS
        body = w[:rows * _SIG_COLS].reshape(rows, _SIG_COLS)
        rest = np.concatenate([w[rows * _SIG_COLS:], b[n8 * 8:].astype(np.uint64)])
        with np.errstate(over="ignore"):
            h_rows = int((body.sum(axis=1, dtype=np.uint64) * _sig_weights(rows, 0)).sum(dtype=np.uint64)) if rows else 0
            h_cols = int((body.sum(axis=0, dtype=np.uint64) * _sig_weights(_SIG_COLS, 1 << 20)).sum(dtype=np.uint64)) if rows else 0
            h_rest = int((rest * _sig_weights(rest.size, 1 << 21)).sum(dtype=np.uint64)) if rest.size else 0
        return (a.shape, str(a.dtype), h_rows, h_cols, h_rest)
    except (TypeError, ValueError, AttributeError):
        return None


class TrackedArray(np.ndarray):
    """The NumPy face of a device-resident model array.  Behaves like the ndarray it is; writing into it (or into a view
    of it) while it is still the model's current snapshot drops the device copy, so that the next kernel sees the edit."""

    _entry = None
    _root = None

    def __array_finalize__(self, obj):
        if obj is not None:
            self._entry = getattr(obj, "_entry", None)
            self._root = getattr(obj, "_root", None)

    def _edited(self):
        ent = self._entry
        if ent is not None and ent.host is not None and ent.host is self._root and ent.dev is not None \
                and np.may_share_memory(self, ent.host):  # a .copy() of the snapshot is the caller's own array
            resolve = getattr(ent.owner, "_resolve_deferred_loss", None)
            if resolve is not None:
                resolve()  # a loss still to be folded into the next pass refers to the state as it was
            ent.dev = None

    def __setitem__(self, key, value):
        self._edited()  # before the write: a deferred loss must still see the old values on the device (it does: dev is intact until dropped)
        super().__setitem__(key, value)

    # the other in-place methods of ndarray
    def fill(self, value):
        self._edited()
        return super().fill(value)

    def sort(self, *args, **kwargs):
        self._edited()
        return super().sort(*args, **kwargs)

    def partition(self, *args, **kwargs):
        self._edited()
        return super().partition(*args, **kwargs)

    def put(self, *args, **kwargs):
        self._edited()
        return super().put(*args, **kwargs)

    def setfield(self, *args, **kwargs):
        self._edited()
        return super().setfield(*args, **kwargs)

    def byteswap(self, inplace=False):
        if inplace:
            self._edited()
        return super().byteswap(inplace)

    # functions of the NumPy API that write into their first argument (np.copyto(a, ..), np.put(a, ..), ...)
    _WRITES_FIRST_ARG = ("copyto", "put", "place", "putmask", "put_along_axis", "fill_diagonal")

    def __array_function__(self, func, types, args, kwargs):
        if getattr(func, "__name__", "") in self._WRITES_FIRST_ARG:
            dst = args[0] if args else kwargs.get("dst", kwargs.get("a", kwargs.get("arr")))
            if isinstance(dst, TrackedArray):
                dst._edited()
        return super().__array_function__(func, types, args, kwargs)

    def __array_ufunc__(self, ufunc, method, *inputs, out=None, **kwargs):
        if method == "at" and inputs and isinstance(inputs[0], TrackedArray):
            inputs[0]._edited()  # np.add.at(a, idx, v) writes into its first input and has no out=
        plain = tuple(np.asarray(x) if isinstance(x, TrackedArray) else x for x in inputs)
        if out is not None:
            for o in out:
                if isinstance(o, TrackedArray):
                    o._edited()
            kwargs["out"] = tuple(o.view(np.ndarray) if isinstance(o, TrackedArray) else o for o in out)
        res = getattr(ufunc, method)(*plain, **kwargs)
        if out is not None:
            return out[0] if len(out) == 1 else out
        return res  # results of arithmetic are plain arrays


class DeviceArray:
    """Descriptor.  get -> NumPy (float64/complex128, batch axis squeezed unless the model is batched);
    raises AttributeError while unset so `hasattr(model, name)` behaves as in the reference."""

    def __init__(self, name, complex_):
        self.name = name
        self.complex_ = complex_

    def __set_name__(self, owner, attr):
        self.attr = attr

    def _store(self, obj):
        return obj.__dict__.setdefault("_arrays", {})

    def __get__(self, obj, objtype=None):
        if obj is None:
            return self
        ent = self._store(obj).get(self.name)
        if ent is None:
            raise AttributeError("'%s' object has no attribute '%s'" % (type(obj).__name__, self.attr))
        if ent.host is None:
            a = to_numpy(ent.dev, np.complex128 if self.complex_ else np.float64)
            a = obj._unbatch(a)
            # in the reference these are plain attributes: `model.demix_filter[...] *= s` takes effect at the next
            # update.  The snapshot is tracked: a write drops the device copy, the next kernel uploads the host array.
            a = a.view(TrackedArray)
            a._entry, a._root = ent, a
            ent.owner = obj
            ent.host = a
            ent.sig = _signature(a)
        return ent.host

    def __set__(self, obj, value):
        resolve = getattr(obj, "_resolve_deferred_loss", None)
        if resolve is not None:
            resolve()  # a loss still to be folded into the next pass refers to the state being replaced
        if isinstance(value, torch.Tensor):
            self._store(obj)[self.name] = _Entry(host=None, dev=None)
            self._store(obj)[self.name].host = to_numpy(value, np.complex128 if self.complex_ else np.float64)
        else:
            self._store(obj)[self.name] = _Entry(host=value, dev=None)

    def __delete__(self, obj):
        self._store(obj).pop(self.name, None)


class DeviceState:
    """Mixin with the device side of DeviceArray attributes."""

    _batched = False

    def _ensure_engine(self):
        if self._engine is None:
            from .ops import Engine  # on first use: importing this module does not import ops
            self._engine = Engine(dtype=self.dtype, device=self.device)
        return self._engine

    # ---- the loop rule ------------------------------------------------------------------------
    _OWN_STEPS = ()  # a model's methods whose override sends the loop back to the Python loop

    def _fast_loop_ok(self):
        """The ONE statement of the rule: the loop goes to the library's one-call `*_iterate` entry only while nothing
        observes the model between iterations -- no callbacks, every step still the model's own (a subclass that
        overrides one keeps the Python loop, which runs what it made of it), and any loss that is recorded goes to the
        list that can hold it on the device.  The model is the first class of the MRO that declares `_OWN_STEPS`; a model
        with further conditions overrides this and calls super() first."""
        if getattr(self, "callbacks", None) is not None:
            return False
        cls = type(self)
        owner = next(c for c in cls.__mro__ if "_OWN_STEPS" in vars(c))
        if not all(getattr(cls, n) is getattr(owner, n) for n in owner._OWN_STEPS):
            return False
        return not getattr(self, "recordable_loss", True) or isinstance(self.loss, LazyLossList)

    def _iterate_block(self, n_entries, touched, call, B=None):
        """One `*_iterate` call: `call(loss)` with the (n_entries, B) float64 block its losses go to (None when they are
        not recorded; a model without `recordable_loss` always records), then the arrays it wrote are `touched` and the
        block joins `loss` without a host sync.  B: the utterances of `_X` unless given.  Returns the block."""
        loss = None
        if getattr(self, "recordable_loss", True):
            loss = self._engine.empty((n_entries, int(self._X.shape[0]) if B is None else B), dtype=torch.float64)
        call(loss)
        self._touch(*touched)
        if loss is not None:
            self.loss.append_device_block(loss, self._batched)
        return loss

    # ---- the front of _reset: refusals before a device is touched, then upload and draws ---------------------------
    def _require_float64(self, dtype, complex_ok=False):
        if str(dtype) not in ('float64', 'double') + (('complex128',) if complex_ok else ()):
            raise ValueError("{} supports float64 only, got dtype={!r}".format(
                getattr(self, "_LABEL", None) or type(self).__name__, dtype))

    def _require_n_basis(self):
        n_basis = self.n_basis
        if not isinstance(n_basis, (int, np.integer)) or not 1 <= n_basis <= self.N_BASIS_MAX:
            raise ValueError("n_basis must be an int in [1, {}], got {!r}".format(self.N_BASIS_MAX, n_basis))
        return n_basis

    @staticmethod
    def _shape_of(x):
        """the shape of an ndarray, a tensor or a nested sequence, as a tuple of ints"""
        return tuple(int(s) for s in x.shape) if hasattr(x, "shape") else np.shape(x)

    def _upload(self, x, dtype):
        """`x` as a contiguous device tensor with the utterance axis in front (added unless the model is batched)."""
        Xd = to_device(x, dtype, self._engine.dev)
        if not self._batched:
            Xd = Xd.unsqueeze(0)
        return Xd.contiguous()

    def _check_warm_start_array(self, attr, want, real=True):
        """Refuses a warm-start array that does not fit the target; returns it, or None while the attribute is absent."""
        if not hasattr(self, attr):
            return None
        a = getattr(self, attr)
        if real and np.iscomplexobj(a):
            raise ValueError("{} supports a real {} only".format(type(self).__name__, attr))
        if tuple(a.shape) != want:
            raise ValueError("{} has shape {}, the target needs {}".format(attr, tuple(a.shape), want))
        return a

    def _keep_or_draw(self, attr, draw, dtype=None):
        """Warm start through `hasattr`, as in the reference: `draw()` runs only while the attribute is absent (the draws
        come from the global RNG, so their number and order are part of the interface); dtype: an existing value is
        replaced by a copy of that type."""
        if not hasattr(self, attr):
            setattr(self, attr, draw())
        elif dtype is not None:
            setattr(self, attr, np.array(getattr(self, attr), dtype=dtype))

    def _unbatch(self, a):
        """a value with the utterance axis in front, as the caller sees it: without it unless the target had one"""
        return a if self._batched else a[0]

    # ---- status ------------------------------------------------------------------------------------------------------
    _SINGULAR_TEXT = "Singular matrix"
    _STATUS_RAISES = _lib.STATUS_SINGULAR  # other flags are informational (STATUS_COND_REJECT) and stay set

    def _check_status(self):
        """Turn device-side flags into the exceptions NumPy would have raised (one sync)."""
        flags = int(self._status.max().item()) & self._STATUS_RAISES
        if flags:
            self._status.zero_()
            if flags & _lib.STATUS_SINGULAR:
                raise np.linalg.LinAlgError(self._SINGULAR_TEXT)
            raise np.linalg.LinAlgError("Eigenvalues did not converge")

    def _has(self, name):
        return name in self.__dict__.get("_arrays", {})

    def _dev(self, name, complex_):
        """Device tensor for `name` (uploads the host value on first use, adding the batch axis)."""
        ent = self.__dict__["_arrays"][name]
        if ent.dev is not None and ent.host is not None and ent.sig is not None and _signature(ent.host) != ent.sig:
            # the host array changed behind the hooks (a write through a plain view of its memory): it is the newer copy
            resolve = getattr(self, "_resolve_deferred_loss", None)
            if resolve is not None:
                resolve()
            ent.dev = None
        if ent.dev is None:
            prec = self._engine.prec
            a = np.asarray(ent.host)
            if not self._batched:
                a = a[None]
            ent.dev = to_device(a, prec.cplx if complex_ else prec.real, self._engine.dev).clone()
            ent.sig = _signature(ent.host)
        return ent.dev

    def _set_dev(self, name, tensor):
        self.__dict__.setdefault("_arrays", {})[name] = _Entry(host=None, dev=tensor)

    def _touch(self, *names):
        """A kernel modified these device tensors: drop the cached NumPy views."""
        arrays = self.__dict__.get("_arrays", {})
        for n in names:
            if n in arrays and arrays[n].dev is not None:
                arrays[n].host = None
