"""0xfec_amd — MI355X-native block FEC engine (the hot path of ddritzenhoff/0xFEC internal/fec).

The compute lives in lib0xfec_hip.so (hand-written gfx950 HIP kernels behind the C ABI of
include/fec_hip.h). This module is a thin ctypes face of that ABI, plus the host-side mirror
of the reference's scheme/manager layer (see `scheme`). There is no CPU fallback: if the
library is missing the import fails, and without a HIP device every compute call raises.

Import by name (the directory starts with a digit):
    fec = importlib.import_module("0xfec_amd")
"""
import ctypes
import functools
import os

# PyTorch-ROCm ships its own libamdhip64.so (same SONAME, libamdhip64.so.7). Loading torch
# first makes the dynamic linker bind this library to that one runtime, so device pointers,
# streams and events are shared with torch; loading ours first would start a second HIP
# runtime in the process, and torch then finds no GPU. Without torch (e.g. a cgo host) the
# library binds to /opt/rocm's runtime.
try:
    import torch as _torch  # noqa: F401
except ImportError:
    _torch = None

from ._build import LIB as _LIB_PATH

# FEC_LIB_PATH selects another build of the same library: the host-ASan/UBSan build
# (0xfec_amd/_san/lib0xfec_hip_san.so) that tests/test_sanitizers.py runs the CPU suite against
_LIB_PATH = os.environ.get("FEC_LIB_PATH") or _LIB_PATH

if not os.path.exists(_LIB_PATH):
    raise ImportError("lib0xfec_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(or python 0xfec_amd/_build.py)")

lib = ctypes.CDLL(_LIB_PATH)

# --- return codes / flags (include/fec_hip.h)
FEC_OK = 0
FEC_ERR_INVALID_ARG = -1
FEC_ERR_INV_SHARD_NUM = -2
FEC_ERR_MAX_SHARD_NUM = -3
FEC_ERR_TOO_FEW_SHARDS = -4
FEC_ERR_SHARD_SIZE = -5
FEC_ERR_SHARD_NO_DATA = -6
FEC_ERR_ALIGNMENT = -7
FEC_ERR_HIP = -8
FEC_ERR_NOMEM = -9
FEC_ERR_NO_DEVICE = -10
FEC_ERR_SINGULAR = -11
FEC_ERR_NO_MATRIX = -12
FEC_DEVICE = 0
FEC_HOST = 1
FEC_HOST_PINNED = 2
FEC_MAX_DECODE_SHARDS = 32
FEC_MAX_WIDE_SHARDS = 256
FEC_LOCATE_CLEAN = -1
FEC_LOCATE_UNKNOWN = -2
FEC_LOCATE_TOO_FEW = -3
FEC_LOCATE_MAX_BAD = 8

_vp = ctypes.c_void_p
_sz = ctypes.c_size_t
_i = ctypes.c_int

lib.fec_version.restype = ctypes.c_char_p
lib.fec_strerror.restype = ctypes.c_char_p
lib.fec_strerror.argtypes = [_i]
lib.fec_device_count.argtypes = [ctypes.POINTER(_i)]
lib.fec_ctx_create.argtypes = [_i, ctypes.POINTER(_vp)]
lib.fec_ctx_destroy.argtypes = [_vp]
lib.fec_ctx_destroy.restype = None
lib.fec_ctx_set_stream.argtypes = [_vp, _vp]
lib.fec_ctx_reset_stream.argtypes = [_vp]
lib.fec_ctx_release_staging.argtypes = [_vp]
lib.fec_ctx_stream.argtypes = [_vp]
lib.fec_ctx_stream.restype = _vp
lib.fec_sync.argtypes = [_vp]
lib.fec_rs_matrix.argtypes = [_i, _i, _vp]
lib.fec_rs_prepare.argtypes = [_vp, _i, _i]
lib.fec_rs_matrix_kind.argtypes = [_i, _i, _i, _vp]
lib.fec_ctx_set_matrix.argtypes = [_vp, _i]
lib.fec_ctx_get_matrix.argtypes = [_vp, ctypes.POINTER(_i)]
lib.fec_ctx_set_custom_matrix.argtypes = [_vp, _i, _i, _vp]
lib.fec_rs_encode_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _i]
lib.fec_rs_reconstruct_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _i]
lib.fec_rs_recover_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _i, _vp, _i]
lib.fec_rs_reconstruct_wide_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _i]
lib.fec_rs_recover_wide_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _vp, _sz, _i, _vp,
                                          _i]
lib.fec_rs_encode_ragged_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _i]
lib.fec_rs_reconstruct_ragged_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _i]
lib.fec_rs_recover_ragged_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _sz, _i, _vp,
                                            _i]
lib.fec_rs_verify_ragged_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _i]
lib.fec_rs_reconstruct_some_ragged_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _vp,
                                                     _i]
lib.fec_rs_verify_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _i]
lib.fec_rs_locate_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _vp, _i]
lib.fec_rs_locate_multi_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _i, _vp, _vp, _sz, _vp, _i]
lib.fec_rs_locate_partial_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _i, _vp, _vp, _vp, _i]
lib.fec_rs_reconstruct_some_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _vp, _i]
lib.fec_rs_reconstruct_some_wide_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _vp,
                                                   _i]
lib.fec_rs_update_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _i]
lib.fec_rs_encode_idx_batch.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _sz, _i]
lib.fec_xor_encode_batch.argtypes = [_vp, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _i]
lib.fec_xor_reconstruct_batch.argtypes = [_vp, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _i]
_u64 = ctypes.c_uint64
lib.fec_synth_data.argtypes = [_vp, _u64, _u64, _sz, _i, _sz, _vp, _sz, _sz]
lib.fec_synth_single_erasures.argtypes = [_vp, _u64, _u64, _sz, _i, _i, _vp, _vp]
lib.fec_probe_encode_traffic.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _i]
lib.fec_probe_recover_traffic.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _i]
lib.fec_probe_rebuild_traffic.argtypes = [_vp, _i, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _vp, _vp, _sz, _i]
lib.fec_probe_stream_traffic.argtypes = [_vp, _i, _sz, _sz, _vp, _sz, _vp, _sz, _sz, _i]
lib.fec_probe_link.argtypes = [_vp, _sz, _i, ctypes.POINTER(ctypes.c_double)]


lib.fec__set_tuning.argtypes = [_vp, _i, _i]
lib.fec__tuning_name.argtypes = [_i]
lib.fec__tuning_name.restype = ctypes.c_char_p


def _tuning_keys():
    keys = {}
    while (name := lib.fec__tuning_name(len(keys))) is not None:
        keys[name.decode()] = len(keys)
    return keys


class FecError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        msg = lib.fec_strerror(code).decode()
        super().__init__("%s%s (code %d)" % (what + ": " if what else "", msg, code))


def _check(rc, what=""):
    if rc != FEC_OK:
        raise FecError(rc, what)
    return rc


def version():
    return lib.fec_version().decode()


def device_count():
    n = _i(0)
    lib.fec_device_count(ctypes.byref(n))
    return n.value


# The matrix kinds (fec_hip_matrix.h): klauspost's default, and its WithCauchyMatrix.
FEC_MATRIX_VANDERMONDE, FEC_MATRIX_CAUCHY = 0, 1
MATRIX_KINDS = {"vandermonde": FEC_MATRIX_VANDERMONDE, "cauchy": FEC_MATRIX_CAUCHY}
# klauspost's WithCustomMatrix: rows registered on a Codec (Codec.set_custom_matrix). No kind of
# MATRIX_KINDS: there is nothing for rs_matrix() to generate.
FEC_MATRIX_CUSTOM = 2


def _matrix_kind(matrix):
    """A kind number from a name of MATRIX_KINDS or a number (unknown numbers are the library's to refuse)."""
    if isinstance(matrix, str):
        if matrix not in MATRIX_KINDS:
            raise ValueError("unknown matrix %r (one of %s)" % (matrix, ", ".join(sorted(MATRIX_KINDS))))
        return MATRIX_KINDS[matrix]
    return int(matrix)


def rs_matrix(k, m, kind=0):
    """n x k systematic matrix of RS(k, m): kind 0 / "vandermonde" klauspost reedsolomon.New's default,
    1 / "cauchy" its WithCauchyMatrix; no device."""
    import numpy as np
    out = np.zeros((k + m, k), dtype=np.uint8)
    kind = _matrix_kind(kind)
    if kind == FEC_MATRIX_VANDERMONDE:
        _check(lib.fec_rs_matrix(k, m, out.ctypes.data), "fec_rs_matrix")
    else:
        _check(lib.fec_rs_matrix_kind(kind, k, m, out.ctypes.data), "fec_rs_matrix_kind")
    return out


def mask_words(n):
    """FEC_MASK_WORDS: the uint32 words a present mask over n shards takes (1..8)."""
    return (n + 31) // 32


def wide_masks(present):
    """bool [B, n] (shard i of block b present) -> uint32 [B, mask_words(n)] numpy array: shard i is
    bit i % 32 of word i // 32, the form the wide calls take."""
    import numpy as np
    present = np.asarray(present, dtype=bool)
    B, n = present.shape
    W = mask_words(n)
    bits = np.zeros((B, W * 32), dtype=np.uint8)
    bits[:, :n] = present
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u4").reshape(B, W)


def _addr(x):
    """(address, memory kind) for a numpy array, a torch tensor, or a raw device address."""
    if isinstance(x, int):
        return x, FEC_DEVICE
    mod = type(x).__module__
    if mod.startswith("numpy"):
        return x.ctypes.data, FEC_HOST
    if mod.startswith("torch"):
        if x.is_cuda:
            return x.data_ptr(), FEC_DEVICE
        return x.data_ptr(), (FEC_HOST_PINNED if x.is_pinned() else FEC_HOST)
    raise TypeError("unsupported buffer type %r" % type(x))


def _shape3(shards):
    B, n, S = shards.shape
    if hasattr(shards, "is_contiguous"):
        assert shards.is_contiguous()
    else:
        assert shards.flags.c_contiguous
    return B, n, S


def _dev(x, what):
    """Address of x, which must lie in device memory (`what`: the assertion's message)."""
    a, kind = _addr(x)
    assert kind == FEC_DEVICE, what
    return a


def _opt(x, dev_only=None):
    """Address of an optional array (None for None); dev_only: as _dev's message."""
    if x is None:
        return None
    return _addr(x)[0] if dev_only is None else _dev(x, dev_only)


_RAGGED = "the ragged calls take device memory only"
_SOME = "verify and reconstruct-some take device memory only"


class _Layout:
    """Where the batch of one call lies, resolved once for both forms of every method: interleaved
    shards [B, k+m, S] (parity None), or split data [B, k, S] and parity [B, m, S] in separate
    buffers of one memory kind. B blocks of S-byte slots, data at address d and parity at p with
    block strides dbs and pbs, memory kind `kind`. dev_only: the message of the assertion that the
    batch lies in device memory, for the calls that take nothing else."""

    def __init__(self, k, m, shards, parity=None, dev_only=None):
        self.B, n, self.S = _shape3(shards)
        self.d, self.kind = _addr(shards)
        if parity is None:
            assert n == k + m
            self.dbs = self.pbs = n * self.S
            self.p = self.d + k * self.S
        else:
            assert n == k and tuple(_shape3(parity)) == (self.B, m, self.S)
            self.dbs, self.pbs = k * self.S, m * self.S
            self.p, pkind = _addr(parity)
            assert pkind == self.kind
        assert dev_only is None or self.kind == FEC_DEVICE, dev_only

    def args(self, shard_len):
        """The C calls' shard_len (default S), nblocks, data, data_block_stride, parity,
        parity_block_stride, shard_stride."""
        return (self.S if shard_len is None else shard_len, self.B, self.d, self.dbs, self.p, self.pbs, self.S)

    def out(self, out, dev_only=None):
        """A recover call's out [B, slots, S]: its address, out_block_stride, out_slots."""
        B, slots, S = _shape3(out)
        assert (B, S) == (self.B, self.S)
        return _opt(out, dev_only), slots * S, slots


class Codec:
    """One device context (one HIP stream). Batch entry points over [B, n, S] uint8 arrays:
    numpy arrays and pageable CPU tensors run the FEC_HOST path (staged through pinned memory),
    pinned CPU tensors the FEC_HOST_PINNED path (direct DMA), CUDA tensors the FEC_DEVICE path
    (asynchronous on the ctx stream; call sync()). matrix: the code matrix of the RS calls,
    "vandermonde" (klauspost's default) or "cauchy" (its WithCauchyMatrix); see set_matrix()."""

    def __init__(self, device=0, matrix="vandermonde"):
        kind = _matrix_kind(matrix)
        h = _vp()
        _check(lib.fec_ctx_create(device, ctypes.byref(h)), "fec_ctx_create")
        self._h = h
        self.device = device
        if kind != FEC_MATRIX_VANDERMONDE:
            self.set_matrix(kind)

    def set_matrix(self, matrix):
        """The matrix kind (a name of MATRIX_KINDS or its number) of every RS call made from now on
        (fec_ctx_set_matrix); legal between calls without a sync. The XOR calls ignore it. "custom" / 2
        switches back to the matrices registered with set_custom_matrix()."""
        kind = FEC_MATRIX_CUSTOM if matrix == "custom" else _matrix_kind(matrix)
        return _check(lib.fec_ctx_set_matrix(self._h, kind), "fec_ctx_set_matrix")

    def set_custom_matrix(self, k, m, rows):
        """Register `rows`, a uint8 [m, k] array of parity rows (klauspost WithCustomMatrix), as the
        code of (k, m) and make "custom" the matrix of the RS calls made from now on
        (fec_ctx_set_custom_matrix); legal between calls without a sync."""
        import numpy as np
        rows = np.ascontiguousarray(rows, dtype=np.uint8)
        if rows.shape != (m, k):
            raise ValueError("rows must be a uint8 [m, k] array, got shape %r" % (rows.shape,))
        return _check(lib.fec_ctx_set_custom_matrix(self._h, k, m, rows.ctypes.data), "fec_ctx_set_custom_matrix")

    @property
    def matrix(self):
        """The name of the ctx's matrix kind (fec_ctx_get_matrix)."""
        kind = _i(-1)
        _check(lib.fec_ctx_get_matrix(self._h, ctypes.byref(kind)), "fec_ctx_get_matrix")
        if kind.value == FEC_MATRIX_CUSTOM:
            return "custom"
        return next(name for name, v in MATRIX_KINDS.items() if v == kind.value)

    def close(self):
        if self._h:
            lib.fec_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def stream(self):
        return lib.fec_ctx_stream(self._h)

    def set_stream(self, stream_ptr):
        """Enqueue on an external hipStream_t (0/None = the null stream)."""
        _check(lib.fec_ctx_set_stream(self._h, stream_ptr or None))

    def reset_stream(self):
        _check(lib.fec_ctx_reset_stream(self._h))

    def use_torch_stream(self):
        """Enqueue on torch's current stream of this device, so codec calls order naturally
        with torch ops on the same tensors."""
        import torch
        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)
        return self

    def sync(self):
        return _check(lib.fec_sync(self._h), "fec_sync")

    def release_staging(self):
        """Free the host-path staging sets (fec_ctx_release_staging); the next host call makes them."""
        return _check(lib.fec_ctx_release_staging(self._h), "fec_ctx_release_staging")

    def lib_sync_rc(self):
        """fec_sync's return code (FEC_ERR_TOO_FEW_SHARDS after a failed block) without raising."""
        return lib.fec_sync(self._h)

    # Tuning knobs (tests and tools; defaults are the measured best): residency of the shipped
    # kernels, routing among shipped kernels, host-path sizes. {name: key} of the library's internal,
    # test-only fec__set_tuning(), read from the library's own list (fec_kernels.hpp
    # FEC_TUNING_KNOBS, through fec__tuning_name()); the setting is process-wide.
    TUNING_KEYS = _tuning_keys()

    def set_tuning(self, **knobs):
        """Set kernel-selection knobs; returns the previous values (pass them back to restore)."""
        old = {}
        for name, val in knobs.items():
            old[name] = lib.fec__set_tuning(self._h, self.TUNING_KEYS[name], int(val))
        return old

    def prepare(self, k, m):
        return _check(lib.fec_rs_prepare(self._h, k, m), "fec_rs_prepare")

    # ---- raw C-ABI mirrors (addresses + strides)
    def rs_encode_raw(self, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, flags):
        return _check(lib.fec_rs_encode_batch(self._h, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, flags),
                      "fec_rs_encode_batch")

    def rs_reconstruct_raw(self, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, masks, status, flags):
        return lib.fec_rs_reconstruct_batch(self._h, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss,
                                            masks, status, flags)

    # ---- array conveniences. Interleaved form: shards is [B, k+m, S]. Split form: data
    # [B, k, S] and parity [B, m, S] in separate buffers. shard_len defaults to S. Each operation
    # is written once, against the _Layout of either form.
    def _encode(self, k, m, lay, shard_len):
        return self.rs_encode_raw(k, m, *lay.args(shard_len), lay.kind)

    def rs_encode(self, k, m, shards, shard_len=None):
        return self._encode(k, m, _Layout(k, m, shards), shard_len)

    def rs_encode_split(self, k, m, data, parity, shard_len=None):
        return self._encode(k, m, _Layout(k, m, data, parity), shard_len)

    def _recon(self, fn, lay, masks, status, shard_len, *mask_words):
        """fn: a C reconstruct call with its arguments before shard_len bound. Returns its return
        code for FEC_OK, FEC_ERR_TOO_FEW_SHARDS and (custom matrices) FEC_ERR_SINGULAR, raises for
        any other."""
        ma, mkind = _addr(masks)
        assert (mkind == FEC_DEVICE) == (lay.kind == FEC_DEVICE), "masks must live where the shards live"
        rc = fn(*lay.args(shard_len), ma, *mask_words, _opt(status), lay.kind)
        if rc not in (FEC_OK, FEC_ERR_TOO_FEW_SHARDS, FEC_ERR_SINGULAR):
            _check(rc, fn.func.__name__)
        return rc

    def _reconstruct(self, k, m, lay, masks, status, shard_len):
        return self._recon(functools.partial(lib.fec_rs_reconstruct_batch, self._h, k, m), lay, masks, status,
                           shard_len)

    def rs_reconstruct(self, k, m, shards, masks, status=None, shard_len=None):
        """Returns the C return code (FEC_OK or FEC_ERR_TOO_FEW_SHARDS for FEC_HOST)."""
        return self._reconstruct(k, m, _Layout(k, m, shards), masks, status, shard_len)

    def rs_reconstruct_split(self, k, m, data, parity, masks, status=None, shard_len=None):
        return self._reconstruct(k, m, _Layout(k, m, data, parity), masks, status, shard_len)

    def rs_recover_raw(self, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, masks, out, out_bs, out_slots,
                       status, flags=FEC_DEVICE):
        return lib.fec_rs_recover_batch(self._h, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, masks,
                                        out, out_bs, out_slots, status, flags)

    def rs_recover_split(self, k, m, data, parity, masks, out, status=None, shard_len=None):
        """Rebuild the erased data shards of each block into out [B, slots, S] (ascending order);
        status[b] = number rebuilt, or a negative error code."""
        lay = _Layout(k, m, data, parity)
        return _check(self.rs_recover_raw(k, m, *lay.args(shard_len), _addr(masks)[0], *lay.out(out), _opt(status)),
                      "fec_rs_recover_batch")

    # ---- wide forms (k + m <= 256): masks are uint32 [B, W] arrays, FEC_MASK_WORDS(k + m) <= W <= 8,
    # living where the shards live; same return conventions as the narrow methods
    def rs_reconstruct_wide_raw(self, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, masks, mask_words,
                                status, flags):
        return lib.fec_rs_reconstruct_wide_batch(self._h, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss,
                                                 masks, mask_words, status, flags)

    def rs_recover_wide_raw(self, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, masks, mask_words, out,
                            out_bs, out_slots, status, flags=FEC_DEVICE):
        return lib.fec_rs_recover_wide_batch(self._h, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, masks,
                                             mask_words, out, out_bs, out_slots, status, flags)

    @staticmethod
    def _mask_shape(masks, B):
        assert len(masks.shape) == 2 and masks.shape[0] == B, "wide masks are [B, W]"
        if hasattr(masks, "is_contiguous"):
            assert masks.is_contiguous() and masks.element_size() == 4
        else:
            assert masks.flags.c_contiguous and masks.itemsize == 4
        return int(masks.shape[1])

    def _reconstruct_wide(self, k, m, lay, masks, status, shard_len):
        return self._recon(functools.partial(lib.fec_rs_reconstruct_wide_batch, self._h, k, m), lay, masks, status,
                           shard_len, self._mask_shape(masks, lay.B))

    def rs_reconstruct_wide(self, k, m, shards, masks, status=None, shard_len=None):
        """Returns the C return code (FEC_OK or FEC_ERR_TOO_FEW_SHARDS for FEC_HOST)."""
        return self._reconstruct_wide(k, m, _Layout(k, m, shards), masks, status, shard_len)

    def rs_reconstruct_wide_split(self, k, m, data, parity, masks, status=None, shard_len=None):
        return self._reconstruct_wide(k, m, _Layout(k, m, data, parity), masks, status, shard_len)

    def rs_recover_wide_split(self, k, m, data, parity, masks, out, status=None, shard_len=None):
        """Rebuild the erased data shards of each block into out [B, slots, S] (ascending order);
        status[b] = number rebuilt, or a negative error code."""
        lay = _Layout(k, m, data, parity)
        W = self._mask_shape(masks, lay.B)
        return _check(self.rs_recover_wide_raw(k, m, *lay.args(shard_len), _addr(masks)[0], W, *lay.out(out),
                                               _opt(status)), "fec_rs_recover_wide_batch")

    # ---- ragged forms (FEC_DEVICE only): lens is a uint32 / int32 device tensor [B], block b's shard
    # length in bytes (0: the block is skipped; > max_shard_len: status FEC_ERR_SHARD_SIZE);
    # max_shard_len defaults to the slot size S. The raw mirrors return the C return code.
    def rs_encode_ragged_raw(self, k, m, max_shard_len, nblocks, data, dbs, parity, pbs, ss, lens, status=None,
                             flags=FEC_DEVICE):
        return lib.fec_rs_encode_ragged_batch(self._h, k, m, max_shard_len, nblocks, data, dbs, parity, pbs, ss,
                                              lens, status, flags)

    def rs_reconstruct_ragged_raw(self, k, m, max_shard_len, nblocks, data, dbs, parity, pbs, ss, masks, lens,
                                  status=None, flags=FEC_DEVICE):
        return lib.fec_rs_reconstruct_ragged_batch(self._h, k, m, max_shard_len, nblocks, data, dbs, parity, pbs, ss,
                                                   masks, lens, status, flags)

    def rs_recover_ragged_raw(self, k, m, max_shard_len, nblocks, data, dbs, parity, pbs, ss, masks, lens, out,
                              out_bs, out_slots, status=None, flags=FEC_DEVICE):
        return lib.fec_rs_recover_ragged_batch(self._h, k, m, max_shard_len, nblocks, data, dbs, parity, pbs, ss,
                                               masks, lens, out, out_bs, out_slots, status, flags)

    @staticmethod
    def _lens_addr(lens, B):
        assert tuple(lens.shape) == (B,) and lens.is_cuda and lens.is_contiguous() and lens.element_size() == 4, \
            "block lengths are a uint32 / int32 device tensor [B]"
        return lens.data_ptr()

    def _encode_ragged(self, k, m, lay, lens, status, max_shard_len):
        return _check(self.rs_encode_ragged_raw(k, m, *lay.args(max_shard_len), self._lens_addr(lens, lay.B),
                                                _opt(status, _RAGGED)), "fec_rs_encode_ragged_batch")

    def rs_encode_ragged(self, k, m, shards, lens, status=None, max_shard_len=None):
        return self._encode_ragged(k, m, _Layout(k, m, shards, None, _RAGGED), lens, status, max_shard_len)

    def rs_encode_ragged_split(self, k, m, data, parity, lens, status=None, max_shard_len=None):
        return self._encode_ragged(k, m, _Layout(k, m, data, parity, _RAGGED), lens, status, max_shard_len)

    def _reconstruct_ragged(self, k, m, lay, masks, lens, status, max_shard_len):
        return _check(self.rs_reconstruct_ragged_raw(k, m, *lay.args(max_shard_len), _dev(masks, _RAGGED),
                                                     self._lens_addr(lens, lay.B), _opt(status, _RAGGED)),
                      "fec_rs_reconstruct_ragged_batch")

    def rs_reconstruct_ragged(self, k, m, shards, masks, lens, status=None, max_shard_len=None):
        return self._reconstruct_ragged(k, m, _Layout(k, m, shards, None, _RAGGED), masks, lens, status,
                                        max_shard_len)

    def rs_reconstruct_ragged_split(self, k, m, data, parity, masks, lens, status=None, max_shard_len=None):
        return self._reconstruct_ragged(k, m, _Layout(k, m, data, parity, _RAGGED), masks, lens, status,
                                        max_shard_len)

    def rs_recover_ragged_split(self, k, m, data, parity, masks, lens, out, status=None, max_shard_len=None):
        """Rebuild the erased data shards of each block into out [B, slots, S] (ascending order);
        status[b] = number rebuilt, or a negative error code."""
        lay = _Layout(k, m, data, parity, _RAGGED)
        return _check(self.rs_recover_ragged_raw(k, m, *lay.args(max_shard_len), _dev(masks, _RAGGED),
                                                 self._lens_addr(lens, lay.B), *lay.out(out, _RAGGED),
                                                 _opt(status, _RAGGED)), "fec_rs_recover_ragged_batch")

    # ---- verify and reconstruct-some (FEC_DEVICE only; device tensors). Verify: status is an int32
    # device tensor [B] (1 = the block's parity matches its data, 0 = not), count an optional
    # uint32 / int32 device tensor of one element that receives the number of bad blocks.
    # Reconstruct-some: masks and want (optional; None = every shard) are uint32 / int32 device
    # tensors [B]; missing parity shards are rebuilt too. The raw mirrors return the C return code.
    def rs_verify_raw(self, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, status, count=None,
                      flags=FEC_DEVICE):
        return lib.fec_rs_verify_batch(self._h, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, status, count,
                                       flags)

    def rs_reconstruct_some_raw(self, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, masks, want=None,
                                status=None, flags=FEC_DEVICE):
        return lib.fec_rs_reconstruct_some_batch(self._h, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss,
                                                 masks, want, status, flags)

    @staticmethod
    def _words_addr(x, count, what):
        assert x.numel() == count and x.is_contiguous() and x.element_size() == 4, \
            "%s is a 4-byte integer device tensor of %d element(s)" % (what, count)
        return _dev(x, _SOME)

    def _verify(self, k, m, lay, status, count, shard_len):
        ca = None if count is None else self._words_addr(count, 1, "count")
        return _check(self.rs_verify_raw(k, m, *lay.args(shard_len), self._words_addr(status, lay.B, "status"), ca),
                      "fec_rs_verify_batch")

    def rs_verify(self, k, m, shards, status, count=None, shard_len=None):
        return self._verify(k, m, _Layout(k, m, shards, None, _SOME), status, count, shard_len)

    def rs_verify_split(self, k, m, data, parity, status, count=None, shard_len=None):
        return self._verify(k, m, _Layout(k, m, data, parity, _SOME), status, count, shard_len)

    # ---- locate (FEC_DEVICE only; device tensors): bad_shard is an int32 device tensor [B] that
    # receives FEC_LOCATE_CLEAN, the corrupt shard's index, or FEC_LOCATE_UNKNOWN per block;
    # present_out an optional 4-byte integer device tensor [B, W], FEC_MASK_WORDS(k + m) <= W <= 8, that
    # receives the present masks which heal the located blocks (W = 1 and k + m <= 32: rs_reconstruct_some's
    # masks, else rs_reconstruct_some_wide's);
    # counts an optional 4-byte integer device tensor of two elements (located, unknown).
    def rs_locate_raw(self, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, bad_shard, present_out=None,
                      mask_words=None, counts=None, flags=FEC_DEVICE):
        return lib.fec_rs_locate_batch(self._h, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, bad_shard,
                                       present_out, (k + m + 31) // 32 if mask_words is None else mask_words, counts,
                                       flags)

    def _locate(self, k, m, lay, bad_shard, present_out, counts, shard_len):
        pa, W = (None, None) if present_out is None else self._col_masks(present_out, lay.B)
        ca = None if counts is None else self._words_addr(counts, 2, "counts")
        return _check(self.rs_locate_raw(k, m, *lay.args(shard_len), self._words_addr(bad_shard, lay.B, "bad_shard"),
                                         pa, W, ca), "fec_rs_locate_batch")

    def rs_locate(self, k, m, shards, bad_shard, present_out=None, counts=None, shard_len=None):
        return self._locate(k, m, _Layout(k, m, shards, None, _SOME), bad_shard, present_out, counts, shard_len)

    def rs_locate_split(self, k, m, data, parity, bad_shard, present_out=None, counts=None, shard_len=None):
        return self._locate(k, m, _Layout(k, m, data, parity, _SOME), bad_shard, present_out, counts, shard_len)

    # ---- locate-multi (FEC_DEVICE only; device tensors; m <= 16): up to min(max_bad, m // 2) corrupt
    # shards per block. bad_count is an int32 device tensor [B] that receives 0, the number of corrupt
    # shards, or FEC_LOCATE_UNKNOWN per block; present_out and counts as for rs_locate, the masks with
    # every located shard's bit cleared.
    def rs_locate_multi_raw(self, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, max_bad, bad_count,
                            present_out=None, mask_words=None, counts=None, flags=FEC_DEVICE):
        return lib.fec_rs_locate_multi_batch(self._h, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, max_bad,
                                             bad_count, present_out,
                                             (k + m + 31) // 32 if mask_words is None else mask_words, counts, flags)

    def _locate_multi(self, k, m, lay, max_bad, bad_count, present_out, counts, shard_len):
        pa, W = (None, None) if present_out is None else self._col_masks(present_out, lay.B)
        ca = None if counts is None else self._words_addr(counts, 2, "counts")
        return _check(self.rs_locate_multi_raw(k, m, *lay.args(shard_len), max_bad,
                                               self._words_addr(bad_count, lay.B, "bad_count"), pa, W, ca),
                      "fec_rs_locate_multi_batch")

    def rs_locate_multi(self, k, m, shards, bad_count, max_bad=FEC_LOCATE_MAX_BAD, present_out=None, counts=None,
                        shard_len=None):
        return self._locate_multi(k, m, _Layout(k, m, shards, None, _SOME), max_bad, bad_count, present_out, counts,
                                  shard_len)

    def rs_locate_multi_split(self, k, m, data, parity, bad_count, max_bad=FEC_LOCATE_MAX_BAD, present_out=None,
                              counts=None, shard_len=None):
        return self._locate_multi(k, m, _Layout(k, m, data, parity, _SOME), max_bad, bad_count, present_out, counts,
                                  shard_len)

    # ---- locate-partial (FEC_DEVICE only; device tensors; m <= 16): rs_locate_multi for blocks that also
    # have missing shards. masks is a 4-byte integer device tensor [B, W] of present
    # masks, FEC_MASK_WORDS(k + m) <= W <= 8; bad_count also receives FEC_LOCATE_TOO_FEW; present_out has
    # the masks' shape and may be masks itself; counts has three elements (located, unknown, too few);
    # max_bad may be 0 (verify only).
    def rs_locate_partial_raw(self, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, present_mask, mask_words,
                              max_bad, bad_count, present_out=None, counts=None, flags=FEC_DEVICE):
        return lib.fec_rs_locate_partial_batch(self._h, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss,
                                               present_mask, mask_words, max_bad, bad_count, present_out, counts,
                                               flags)

    def _locate_partial(self, k, m, lay, masks, max_bad, bad_count, present_out, counts, shard_len):
        ma, W = self._col_masks(masks, lay.B)
        pa = None
        if present_out is not None:
            pa, Wo = self._col_masks(present_out, lay.B)
            assert Wo == W, "present_out has the masks' shape"
        ca = None if counts is None else self._words_addr(counts, 3, "counts")
        return _check(self.rs_locate_partial_raw(k, m, *lay.args(shard_len), ma, W, max_bad,
                                                 self._words_addr(bad_count, lay.B, "bad_count"), pa, ca),
                      "fec_rs_locate_partial_batch")

    def rs_locate_partial(self, k, m, shards, masks, bad_count, max_bad=FEC_LOCATE_MAX_BAD, present_out=None,
                          counts=None, shard_len=None):
        return self._locate_partial(k, m, _Layout(k, m, shards, None, _SOME), masks, max_bad, bad_count, present_out,
                                    counts, shard_len)

    def rs_locate_partial_split(self, k, m, data, parity, masks, bad_count, max_bad=FEC_LOCATE_MAX_BAD,
                                present_out=None, counts=None, shard_len=None):
        return self._locate_partial(k, m, _Layout(k, m, data, parity, _SOME), masks, max_bad, bad_count, present_out,
                                    counts, shard_len)

    def _reconstruct_some(self, k, m, lay, masks, want, status, shard_len):
        wa = None if want is None else self._words_addr(want, lay.B, "want")
        sa = None if status is None else self._words_addr(status, lay.B, "status")
        return _check(self.rs_reconstruct_some_raw(k, m, *lay.args(shard_len),
                                                   self._words_addr(masks, lay.B, "masks"), wa, sa),
                      "fec_rs_reconstruct_some_batch")

    def rs_reconstruct_some(self, k, m, shards, masks, want=None, status=None, shard_len=None):
        return self._reconstruct_some(k, m, _Layout(k, m, shards, None, _SOME), masks, want, status, shard_len)

    def rs_reconstruct_some_split(self, k, m, data, parity, masks, want=None, status=None, shard_len=None):
        return self._reconstruct_some(k, m, _Layout(k, m, data, parity, _SOME), masks, want, status, shard_len)

    # ---- ragged verify and reconstruct-some (include/fec_hip_ragged.h; FEC_DEVICE only): the two calls
    # above with lens, a uint32 / int32 device tensor [B], as the other ragged forms take it;
    # max_shard_len defaults to the slot size S. A block longer than max_shard_len gets status
    # FEC_ERR_SHARD_SIZE. The raw mirrors return the C return code.
    def rs_verify_ragged_raw(self, k, m, max_shard_len, nblocks, data, dbs, parity, pbs, ss, lens, status, count=None,
                             flags=FEC_DEVICE):
        return lib.fec_rs_verify_ragged_batch(self._h, k, m, max_shard_len, nblocks, data, dbs, parity, pbs, ss, lens,
                                              status, count, flags)

    def rs_reconstruct_some_ragged_raw(self, k, m, max_shard_len, nblocks, data, dbs, parity, pbs, ss, masks, lens,
                                       want=None, status=None, flags=FEC_DEVICE):
        return lib.fec_rs_reconstruct_some_ragged_batch(self._h, k, m, max_shard_len, nblocks, data, dbs, parity, pbs,
                                                        ss, masks, want, lens, status, flags)

    def _verify_ragged(self, k, m, lay, lens, status, count, max_shard_len):
        ca = None if count is None else self._words_addr(count, 1, "count")
        return _check(self.rs_verify_ragged_raw(k, m, *lay.args(max_shard_len), self._lens_addr(lens, lay.B),
                                                self._words_addr(status, lay.B, "status"), ca),
                      "fec_rs_verify_ragged_batch")

    def rs_verify_ragged(self, k, m, shards, lens, status, count=None, max_shard_len=None):
        return self._verify_ragged(k, m, _Layout(k, m, shards, None, _RAGGED), lens, status, count, max_shard_len)

    def rs_verify_ragged_split(self, k, m, data, parity, lens, status, count=None, max_shard_len=None):
        return self._verify_ragged(k, m, _Layout(k, m, data, parity, _RAGGED), lens, status, count, max_shard_len)

    def _reconstruct_some_ragged(self, k, m, lay, masks, lens, want, status, max_shard_len):
        wa = None if want is None else self._words_addr(want, lay.B, "want")
        sa = None if status is None else self._words_addr(status, lay.B, "status")
        return _check(self.rs_reconstruct_some_ragged_raw(k, m, *lay.args(max_shard_len),
                                                          self._words_addr(masks, lay.B, "masks"),
                                                          self._lens_addr(lens, lay.B), wa, sa),
                      "fec_rs_reconstruct_some_ragged_batch")

    def rs_reconstruct_some_ragged(self, k, m, shards, masks, lens, want=None, status=None, max_shard_len=None):
        return self._reconstruct_some_ragged(k, m, _Layout(k, m, shards, None, _RAGGED), masks, lens, want, status,
                                             max_shard_len)

    def rs_reconstruct_some_ragged_split(self, k, m, data, parity, masks, lens, want=None, status=None,
                                         max_shard_len=None):
        return self._reconstruct_some_ragged(k, m, _Layout(k, m, data, parity, _RAGGED), masks, lens, want, status,
                                             max_shard_len)

    # ---- wide reconstruct-some (include/fec_hip_some_wide.h; FEC_DEVICE only; k + m <= 256): masks and want
    # (optional; None = every shard) are 4-byte integer device tensors [B, W] of one shape,
    # FEC_MASK_WORDS(k + m) <= W <= 8 (wide_masks() builds them); the masks the locate calls write into
    # present_out are the masks to pass. The raw mirror returns the C return code.
    def rs_reconstruct_some_wide_raw(self, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, masks, mask_words,
                                     want=None, status=None, flags=FEC_DEVICE):
        return lib.fec_rs_reconstruct_some_wide_batch(self._h, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss,
                                                      masks, want, mask_words, status, flags)

    def _reconstruct_some_wide(self, k, m, lay, masks, want, status, shard_len):
        ma, W = self._col_masks(masks, lay.B)
        wa = None
        if want is not None:
            wa, Ww = self._col_masks(want, lay.B)
            assert Ww == W, "want has the masks' shape"
        sa = None if status is None else self._words_addr(status, lay.B, "status")
        return _check(self.rs_reconstruct_some_wide_raw(k, m, *lay.args(shard_len), ma, W, wa, sa),
                      "fec_rs_reconstruct_some_wide_batch")

    def rs_reconstruct_some_wide(self, k, m, shards, masks, want=None, status=None, shard_len=None):
        return self._reconstruct_some_wide(k, m, _Layout(k, m, shards, None, _SOME), masks, want, status, shard_len)

    def rs_reconstruct_some_wide_split(self, k, m, data, parity, masks, want=None, status=None, shard_len=None):
        return self._reconstruct_some_wide(k, m, _Layout(k, m, data, parity, _SOME), masks, want, status, shard_len)

    # ---- update and encode-idx (klauspost Update / EncodeIdx; FEC_DEVICE only; device tensors): parity
    # is changed in place by the columns each block's mask names. masks is a 4-byte integer device
    # tensor [B, W], FEC_MASK_WORDS(k) <= W <= 8, column j = bit j % 32 of word j // 32 (wide_masks()
    # builds it). Neither call copies new data over old. The raw mirrors return the C return code.
    def rs_update_raw(self, k, m, shard_len, nblocks, old, old_bs, new, new_bs, parity, pbs, ss, masks, mask_words,
                      flags=FEC_DEVICE):
        return lib.fec_rs_update_batch(self._h, k, m, shard_len, nblocks, old, old_bs, new, new_bs, parity, pbs, ss,
                                       masks, mask_words, flags)

    def rs_encode_idx_raw(self, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, masks, mask_words,
                          flags=FEC_DEVICE):
        return lib.fec_rs_encode_idx_batch(self._h, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, masks,
                                           mask_words, flags)

    def _col_masks(self, masks, B):
        W = self._mask_shape(masks, B)
        return _dev(masks, _SOME), W

    def _update(self, k, m, lay, new, masks, shard_len):
        assert tuple(_shape3(new)) == (lay.B, k, lay.S)
        L, B, old, old_bs, parity, pbs, S = lay.args(shard_len)
        return _check(self.rs_update_raw(k, m, L, B, old, old_bs, _dev(new, _SOME), k * S, parity, pbs, S,
                                         *self._col_masks(masks, B)), "fec_rs_update_batch")

    def rs_update(self, k, m, shards, new_data, masks, shard_len=None):
        """shards [B, k+m, S] holds the old data and the parity (changed in place), new_data [B, k, S]."""
        return self._update(k, m, _Layout(k, m, shards, None, _SOME), new_data, masks, shard_len)

    def rs_update_split(self, k, m, old, new, parity, masks, shard_len=None):
        return self._update(k, m, _Layout(k, m, old, parity, _SOME), new, masks, shard_len)

    def _encode_idx(self, k, m, lay, masks, shard_len):
        return _check(self.rs_encode_idx_raw(k, m, *lay.args(shard_len), *self._col_masks(masks, lay.B)),
                      "fec_rs_encode_idx_batch")

    def rs_encode_idx(self, k, m, shards, masks, shard_len=None):
        """shards [B, k+m, S]: the masked data columns are folded into the parity slots."""
        return self._encode_idx(k, m, _Layout(k, m, shards, None, _SOME), masks, shard_len)

    def rs_encode_idx_split(self, k, m, data, parity, masks, shard_len=None):
        return self._encode_idx(k, m, _Layout(k, m, data, parity, _SOME), masks, shard_len)

    # ---- synthetic workload on the device (include/fec_synth.h; same bytes as shard.py)
    def synth_data(self, seed, first_block, nblocks, k, payload_len, data, block_stride, shard_stride):
        """Fill data shards of global blocks [first_block, first_block + nblocks) at the device
        address `data` (asynchronous on the ctx stream)."""
        return _check(lib.fec_synth_data(self._h, seed, first_block, nblocks, k, payload_len, data, block_stride,
                                         shard_stride), "fec_synth_data")

    def synth_single_erasures(self, seed, first_block, nblocks, k, m, masks, erased=None):
        return _check(lib.fec_synth_single_erasures(self._h, seed, first_block, nblocks, k, m, masks, erased),
                      "fec_synth_single_erasures")

    # ---- traffic twins of the headline kernels (include/fec_probe.h; measurement only). wpc:
    # resident workgroups per CU (-1: the twinned kernel's own, 0: as many as fit)
    def probe_encode_traffic_raw(self, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, wpc=-1):
        return _check(lib.fec_probe_encode_traffic(self._h, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, wpc),
                      "fec_probe_encode_traffic")

    def probe_recover_traffic_raw(self, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, masks, out, out_bs,
                                  wpc=-1):
        return _check(lib.fec_probe_recover_traffic(self._h, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss,
                                                    masks, out, out_bs, wpc), "fec_probe_recover_traffic")

    def probe_rebuild_traffic_raw(self, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss, masks, out, out_bs,
                                  wpc=-1):
        return _check(lib.fec_probe_rebuild_traffic(self._h, k, m, shard_len, nblocks, data, dbs, parity, pbs, ss,
                                                    masks, out, out_bs, wpc), "fec_probe_rebuild_traffic")

    def probe_stream_traffic_raw(self, nin, shard_len, nblocks, data, in_bs, out, out_bs, ss, wpc=0):
        return _check(lib.fec_probe_stream_traffic(self._h, nin, shard_len, nblocks, data, in_bs, out, out_bs, ss, wpc),
                      "fec_probe_stream_traffic")

    def probe_link(self, nbytes=512 << 20, reps=3):
        """{h2d, d2h, duplex_each} GB/s of pinned hipMemcpyAsync on this ctx's device."""
        out = (ctypes.c_double * 3)()
        _check(lib.fec_probe_link(self._h, nbytes, reps, out), "fec_probe_link")
        return {"bytes": nbytes, "h2d_GBps": round(out[0], 2), "d2h_GBps": round(out[1], 2),
                "duplex_each_GBps": round(out[2], 2)}

    def xor_encode(self, k, shards, shard_len=None):
        lay = _Layout(k, 1, shards)
        return _check(lib.fec_xor_encode_batch(self._h, k, *lay.args(shard_len), lay.kind), "fec_xor_encode_batch")

    def xor_reconstruct(self, k, shards, masks, status=None, shard_len=None):
        return self._recon(functools.partial(lib.fec_xor_reconstruct_batch, self._h, k), _Layout(k, 1, shards), masks,
                           status, shard_len)

