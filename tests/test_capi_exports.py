"""The C-ABI library loads and exports every entry point its public headers declare (no GPU:
no compute call is made)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fec_[a-z0-9_]+)\s*\(", src)))


def test_headers_declare_entry_points():
    names = declared("fec_hip.h")
    for want in ["fec_ctx_create", "fec_rs_encode_batch", "fec_rs_reconstruct_batch",
                 "fec_xor_encode_batch", "fec_xor_reconstruct_batch", "fec_sync", "fec_strerror"]:
        assert want in names


def test_library_exports_every_declared_symbol(fec):
    lib = ctypes.CDLL(fec._LIB_PATH)
    headers = [h for h in os.listdir(os.path.join(ROOT, "include")) if h.endswith(".h")]
    missing = []
    for h in headers:
        for name in declared(h):
            if not hasattr(lib, name):
                missing.append((h, name))
    assert not missing, missing


def test_no_device_needed_for_host_helpers(fec):
    assert fec.version().startswith("0xfec")
    assert fec.lib.fec_strerror(fec.FEC_ERR_TOO_FEW_SHARDS) == b"too few shards given"
    m = fec.rs_matrix(8, 4)
    assert bytes(m[8]).hex() == "1a84ba33e710c627"
    assert (m[:8] == np.eye(8, dtype=np.uint8)).all()


def test_matrix_matches_oracle(fec, oracle):
    for k, m in [(1, 1), (2, 1), (6, 2), (8, 4), (16, 8), (20, 10), (3, 29), (100, 156)]:
        assert np.array_equal(fec.rs_matrix(k, m), oracle.build_matrix(k, k + m)), (k, m)


def test_shard_count_errors_without_device(fec):
    import pytest
    with pytest.raises(fec.FecError) as e:
        fec.rs_matrix(0, 1)
    assert e.value.code == fec.FEC_ERR_INV_SHARD_NUM
    with pytest.raises(fec.FecError) as e:
        fec.rs_matrix(200, 57)
    assert e.value.code == fec.FEC_ERR_MAX_SHARD_NUM


def test_context_fails_loudly_without_gpu(fec):
    """No CPU fallback: with no HIP device the context cannot be created."""
    import pytest
    if fec.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(fec.FecError) as e:
        fec.Codec(0)
    assert e.value.code == fec.FEC_ERR_NO_DEVICE


def test_lane_permtab_builder_matches_bytewise(fec):
    # the rebuild kernels expand coefficient rows with gf::make_permtab_fast (32-bit lane
    # arithmetic, v_perm byte moves restated on the host); it must equal the byte-wise table
    # builder for all 256 coefficients
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_permtab() == 0


def test_copy_workers_cover_every_index_once(fec):
    # FEC_HOST's staging / scatter copies run through parallel_for on persistent copy workers
    # (fec_host.cpp CopyPool) or on threads made per call: every index exactly once, for sizes
    # around the part boundaries, 2..16 parts, four callers at once (no device needed; the
    # sanitized CPU run repeats it under ASan / UBSan)
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_copypool() == 0


def test_store_policy_follows_region_hulls(fec):
    # sc1 stores only into a parity (or out) region apart from the shards read: the library's
    # table of layouts (fec_selftest.cpp fec__selftest_store_policy): split block-major and
    # shard-major in one region apart, interleaved and row-alternating shard-major not, empty
    # batches nt, knob st_pol 2 sc1 always (no device needed: addresses are only compared)
    lib = ctypes.CDLL(fec._LIB_PATH)
    assert lib.fec__selftest_store_policy() == 0


def test_batch_calls_check_arguments_in_the_documented_order(fec):
    """Every check of the 13 batch entry points that runs before the ctx is looked at, by calling
    them with a null ctx (no device needed): the shard counts, then k + m against the call's limit,
    then the flags the call accepts, then shard_len (0, then above 2^30), then out_slots and
    mask_words (fec_hip.h); pairs of bad arguments pin which check wins. Arguments that pass them
    all reach the ctx check: FEC_ERR_INVALID_ARG."""
    from capi_calls import CALLS, layout
    INV, NUM, MAX, NODATA = (fec.FEC_ERR_INVALID_ARG, fec.FEC_ERR_INV_SHARD_NUM, fec.FEC_ERR_MAX_SHARD_NUM,
                             fec.FEC_ERR_SHARD_NO_DATA)
    for call in CALLS:
        F = getattr(fec.lib, call.name)
        has = lambda f: f in call.tail   # noqa: E731
        over = dict(k=call.max_n) if call.xor else dict(k=call.max_n - 1, m=2)   # k + m one above the limit
        host = INV if not call.host else None   # a host flag: refused, or on to the next check
        cases = [
            ({}, INV),
            (dict(k=0), NUM), (dict(k=-1), NUM), (over, MAX),
            (dict(k=call.max_n - 1, m=1), INV),   # the limit itself passes
            (dict(flags=3), INV), (dict(flags=-1), INV), (dict(flags=1), INV), (dict(flags=2), INV),
            (dict(shard_len=0), NODATA), (dict(shard_len=(1 << 30) + 1), INV), (dict(shard_len=1 << 30), INV),
            (dict(k=0, **{f: v for f, v in over.items() if f != "k"}), NUM),
            (dict(k=0, flags=3), NUM), (dict(k=0, shard_len=0), NUM),
            (dict(flags=3, **over), MAX), (dict(shard_len=0, **over), MAX),
            (dict(flags=3, shard_len=0), INV),
            (dict(flags=1, shard_len=0), host or NODATA), (dict(flags=2, shard_len=0), host or NODATA),
        ]
        if not call.xor:
            cases += [(dict(m=-1), NUM), (dict(k=300, m=-1), NUM), (dict(m=-1, flags=3), NUM),
                      (dict(m=-1, shard_len=0), NUM)]
        if has("out_slots"):
            cases += [(dict(out_slots=0), INV), (dict(out_slots=-1), INV), (dict(out_slots=0, shard_len=0), NODATA),
                      (dict(out_slots=0, **over), MAX)]
        if has("mask_words"):
            cases += [(dict(mask_words=0), INV), (dict(mask_words=9), INV), (dict(k=30, m=10, mask_words=1), INV),
                      (dict(k=200, m=56, mask_words=7), INV), (dict(k=200, m=56, mask_words=8), INV),
                      (dict(mask_words=9, shard_len=0), NODATA), (dict(mask_words=9, flags=3), INV),
                      (dict(mask_words=9, k=0), NUM), (dict(mask_words=9, **over), MAX),
                      # one word and a narrow code: the forward to the narrow call, same codes
                      (dict(mask_words=1), INV), (dict(mask_words=1, shard_len=0), NODATA),
                      (dict(mask_words=2, shard_len=0), NODATA)]
        for over_v, want in cases:
            v = dict(ctx=None, k=3, m=2, shard_len=17, nblocks=1, data=None, data_bs=0, parity=None, parity_bs=0,
                     ss=32, mask=None, status=None, lens=None, want=None, count=None, out=None, out_bs=0,
                     out_slots=1, mask_words=1, flags=fec.FEC_DEVICE)
            v.update(over_v)
            assert F(*layout(call, v)) == want, (call.name, over_v)
