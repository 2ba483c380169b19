"""Shards past 256 chunks through every core kernel, bit-exact against the CPU oracle (and, for codes
wider than 32 shards, the inverse-matrix reference of test_gpu_wide.py).

The rest of the device suite gives these kernels shards of at most 1436 bytes (90 chunks of 16), so one
block never spans more than one 256-lane workgroup there. Here a shard has 257 chunks (4099 bytes, a
3-byte tail) or 4375 (69 989 bytes, a 5-byte tail): many consecutive workgroups lie inside one block,
the block edge moves through the wave from block to block, the wide tile meets a nonzero chunk tile,
and the workgroup-tile rebuild one block of more than 8 rounds. The cases (long_shard_cases.py) are
tiny in blocks; test_long_shard_cases.py checks them without a device. Section 5 runs batches that the
launch limit cuts in two.

Every comparison is of whole arenas (arena.py, test_gpu_layouts.py): the image before the call with
only the bytes the header lets the call write changed.
"""
import numpy as np
import pytest

import long_shard_cases as lc
from arena import CANARY, GUARD, MUL, check_arena, codec, rup16, torch  # noqa: F401
from test_gpu_codec import DEC_VARIANTS, ENC_VARIANTS, ROUTE_FORMS
from test_gpu_layouts import expect_sync, run_rs_step, run_xor
from test_gpu_some import run_some
from test_gpu_wide import run_wide, run_wide_arena

pytestmark = pytest.mark.gpu

ERASED = lc.ERASED
L_SHORT, L_LONG = lc.L_SHORT, lc.L_LONG

# ------------------------------------------------------------------ 1. narrow RS
# What the dispatch (fec_cores.cpp rs_encode_device / rs_reconstruct_device, fec_encode.hip,
# fec_recover.hip) selects for each code at 257 chunks and more, default knobs:
#   (2,1)    encode: fec_encode23 (rs_encode23_kernel). m = 1, so every decode is direct:
#            rs_recover_k2m1_kernel (rows by kernel argument); "table": direct<2, 0>.
#   (8,4)    encode: the dyadic rs_encode_fixed_kernel<8, 4>: three working waves and sc1 stores where
#            the parity region lies apart from the data (split_parity_first), nt stores and four waves
#            where it does not (interleaved_slack); "ww4": four waves with sc1 stores; "stpol_nt": nt
#            stores on both layouts. In place: rs_reconstruct_routed_kernel<4, 8, 1, 0, 3> after the
#            classify pass. recover_1: direct<8, 1, 3> (the out arena lies apart). recover_m: sorted
#            plans + rs_reconstruct_wave_kernel<4>.
#   (8,8)    encode: generic rs_encode_kernel<8, true>. In place: the routed kernel's <8, 8, ...>
#            instances. recover_1: direct<8, 1, 3> (its 128 coefficient words just fit the argument).
#            recover_m: sorted plans + wave<8>.
#   (16,8)   encode: bit-sliced rs_encode_bits_kernel<16, 8> (items in pairs). In place and
#   (20,10)  recover_m: sorted plans + rs_rebuild_k_kernel<16, 8, 4> / <20, 10, 6>. recover_1:
#            direct<16, 2> / direct<20, 2> (rows from the device table).
#   (6,2)    encode: generic <2, true> (tables in LDS). recover_1: direct<0, 1> (runtime k). In place
#            and recover_m: sorted plans + wave<2>.
#   (10,22)  encode: generic in two row passes, <16, true> and <8, true>. n = 32, maxe = 10, no direct
#            table (k * m * k PermTabs exceed 16 KiB): sorted plans + wave<16> for every step.
#   (31,1)   encode: generic <1, true>. Its single-erasure table (31 * 31 PermTabs, 30 KiB) exceeds
#            the direct kernels' 16 KiB, so no direct body runs although m = 1: sorted plans +
#            wave<1>, four input groups of 8 per item (recon_item), for every step.
# Knob variants (names of test_gpu_codec.py): "plan" (dec_direct 0) sends every code through the sorted
# plans and the wave form, or rs_rebuild_k_kernel for (16,8) / (20,10); "tile" (dec_direct 0, dec_wave
# 0) through rs_plan_kernel and the workgroup-tile rs_reconstruct_kernel, where pick_tile_blocks gives
# 7 blocks per tile at 257 chunks (8 rounds of 256 items; the 11 blocks make tiles of 7 and 4) and its
# g == 1 && rounds > kMaxRounds case, one block of 18 rounds, at 4375; "table" (dec_direct 2) makes the
# direct kernels copy their rows from the PermTab table (TAB 0; (16,8) / (20,10) keep TAB 2) and takes
# (8,4) / (8,8) in place off the routed form; "generic" (enc_fixed 0) is rs_encode_kernel for every code.

DEC_NAMES = ["default", "plan", "tile", "table"]
ENC_NAMES = ["own", "generic", "ww4", "stpol_nt"]
STEPS = ["reconstruct", "recover_m", "recover_1"]
# (8,4) in place: the default routed form, the sorted-plan route for every batch, and the routed form
# with all four waves on its direct route
ROUTES = {"routed": ROUTE_FORMS[1], "noroute": DEC_VARIANTS["noroute"], "route_ww4": ROUTE_FORMS[2]}


@pytest.mark.parametrize("variant", ENC_NAMES)
@pytest.mark.parametrize("layout", lc.NARROW_LAYOUTS)
@pytest.mark.parametrize("k,m", lc.NARROW_CODES)
def test_narrow_encode_257_chunks(codec, oracle, torch, fec, tune, k, m, layout, variant):
    tune(**ENC_VARIANTS[variant])
    run_rs_step(codec, fec, torch, lc.narrow_case(oracle, k, m, L_SHORT), layout, k, m, L_SHORT, "encode")


@pytest.mark.parametrize("variant", DEC_NAMES)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("layout", lc.NARROW_LAYOUTS)
@pytest.mark.parametrize("k,m", lc.NARROW_CODES)
def test_narrow_decode_257_chunks(codec, oracle, torch, fec, tune, k, m, layout, step, variant):
    tune(**DEC_VARIANTS[variant])
    run_rs_step(codec, fec, torch, lc.narrow_case(oracle, k, m, L_SHORT), layout, k, m, L_SHORT, step)


@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("L,layout", [(L_SHORT, "interleaved_slack"), (L_SHORT, "split_parity_first"),
                                      (L_LONG, "interleaved_slack")])
def test_rs_8_4_in_place_routes(codec, oracle, torch, fec, tune, L, layout, route, multi):
    """RS(8,12) in place with single-erasure blocks only (the route word stays zero: the routed
    kernel's direct body) and with multi-erasure blocks mixed in (nonzero: its wave rebuild)."""
    k, m = 8, 4
    c = lc.narrow_case(oracle, k, m, L, single_only=not multi)
    assert (c["e_d"][~c["few"]] >= 2).any() == multi
    tune(**ROUTES[route])
    run_rs_step(codec, fec, torch, c, layout, k, m, L, "reconstruct")


@pytest.mark.parametrize("variant", ["own", "generic"])
@pytest.mark.parametrize("k,m", lc.NARROW_LONG_CODES)
def test_narrow_encode_4375_chunks(codec, oracle, torch, fec, tune, k, m, variant):
    tune(**ENC_VARIANTS[variant])
    run_rs_step(codec, fec, torch, lc.narrow_case(oracle, k, m, L_LONG), "interleaved_slack", k, m, L_LONG, "encode")


@pytest.mark.parametrize("variant", ["default", "tile"])
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("k,m", lc.NARROW_LONG_CODES)
def test_narrow_decode_4375_chunks(codec, oracle, torch, fec, tune, k, m, step, variant):
    tune(**DEC_VARIANTS[variant])
    run_rs_step(codec, fec, torch, lc.narrow_case(oracle, k, m, L_LONG), "interleaved_slack", k, m, L_LONG, step)


@pytest.mark.parametrize("L", lc.LENS)
@pytest.mark.parametrize("k,m", lc.WIDE_ENCODES)
def test_wide_encode_long_shards(codec, oracle, torch, k, m, L):
    """Parity only, as test_rs_wide_encode_matches_oracle: (5,20) takes two parity row passes, (130,20)
    reads its first pass's tables (16 * 130 > 2048 PermTabs) from global memory."""
    ref = lc.wide_encode_case(oracle, k, m, L)
    B, S = lc.WIDE_B, rup16(L)
    data = np.full((B, k, S), CANARY, dtype=np.uint8)    # input slots hold canary from L on
    data[:, :, :L] = ref[:, :k]
    want = np.zeros((B, m, S), dtype=np.uint8)
    want[:, :, :L] = ref[:, k:]
    d = torch.from_numpy(data).cuda()
    p = torch.full((B, m, S), 0xA5, dtype=torch.uint8, device="cuda")
    codec.rs_encode_split(k, m, d, p, shard_len=L)
    codec.sync()
    assert np.array_equal(p.cpu().numpy(), want)
    assert np.array_equal(d.cpu().numpy(), data)


# ------------------------------------------------------------------ 2. the wide rebuild kernel past one chunk tile
# rs_rebuild_wide_kernel takes tiles of g blocks x c chunks with c = min(cps, 256): at 257 chunks two
# chunk tiles per block (the second with one live lane), at 4375 eighteen (the last with 23), one block
# per tile. (40,20) with 20 and (128,128) with 21 lost data shards take a second row pass over them.

WIDE_RUNS = [(k, m, L) for L in lc.LENS for (k, m) in lc.WIDE_CODES[L]]


@pytest.mark.parametrize("k,m,L", WIDE_RUNS)
def test_wide_reconstruct_long_shards(fec, codec, oracle, torch, MUL, k, m, L):
    c = lc.wide_case(oracle, fec, MUL, k, m, L)
    got, st, sync = run_wide(fec, codec, torch, k, m, c["dmg"].copy(), c["masks"].copy(), L)
    assert np.array_equal(st, c["st_ref"])
    assert np.array_equal(got, c["ref"])
    assert np.array_equal(got[:2, :k, :L], c["sh"][:2, :k, :L])
    assert sync == fec.FEC_ERR_TOO_FEW_SHARDS


@pytest.mark.parametrize("one_slot", [True, False])
@pytest.mark.parametrize("k,m,L", WIDE_RUNS)
def test_wide_recover_long_shards(fec, codec, oracle, torch, MUL, k, m, L, one_slot):
    """Into one slot (the block that lost many reports -1) and into min(k, m) slots; slots of
    round_up(L, 16) + 16 bytes, canary wherever the call may not write."""
    c = lc.wide_case(oracle, fec, MUL, k, m, L)
    B, R = lc.WIDE_B, rup16(L)
    S = R + 16
    slots = 1 if one_slot else min(k, m)
    present, es = c["present"], c["es"]
    dmg = np.full((B, k + m, S), CANARY, dtype=np.uint8)   # input slots hold canary from L on
    dmg[:, :, :L] = c["dmg"][:, :, :L]
    dd, dp = torch.from_numpy(dmg[:, :k].copy()).cuda(), torch.from_numpy(dmg[:, k:].copy()).cuda()
    dm = torch.from_numpy(c["masks"].copy().view(np.int32)).cuda()
    out = torch.full((B, slots, S), CANARY, dtype=torch.uint8, device="cuda")
    ds = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_recover_wide_split(k, m, dd, dp, dm, out, status=ds, shard_len=L)
    sync = codec.lib_sync_rc()
    want_st = np.array([e if e <= slots else -1 for e in es] + [-4], dtype=np.int32)
    assert np.array_equal(ds.cpu().numpy(), want_st)
    assert sync == fec.FEC_ERR_TOO_FEW_SHARDS
    model = np.full((B, slots, S), CANARY, dtype=np.uint8)
    for b in np.flatnonzero(want_st > 0):
        lost = np.flatnonzero(~present[b, :k])   # ascending
        model[b, :len(lost), :L] = c["ref"][b, lost, :L]
        model[b, :len(lost), L:R] = 0
    assert (want_st > 0).any()
    assert np.array_equal(out.cpu().numpy(), model)
    assert np.array_equal(dd.cpu().numpy(), dmg[:, :k]) and np.array_equal(dp.cpu().numpy(), dmg[:, k:])


@pytest.mark.parametrize("layout", ["interleaved_slack", "shard_major"])
def test_wide_calls_write_only_their_output_bytes_257_chunks(fec, codec, oracle, torch, layout):
    """The whole-arena runner of test_gpu_wide.py, RS(40,20) recover and reconstruct, 11 blocks that hold
    every one of its eight kinds."""
    run_wide_arena(fec, codec, oracle, torch, layout, L_SHORT, lc.WIDE_ARENA_B)


@pytest.mark.parametrize("L", lc.LENS)
@pytest.mark.parametrize("k,m", lc.SOME_CODES)
def test_reconstruct_some_everything_long_shards(codec, oracle, torch, fec, k, m, L):
    """want = NULL: every missing shard of every recoverable block; lost parity is rebuilt byte for
    byte as the oracle's encode makes it."""
    c = lc.some_case(oracle, k, m, L)
    _, _, st, rebuilt, _ = run_some(codec, fec, torch, c, "interleaved_slack", k, m, L)
    assert (st == -4).any() and rebuilt[:, k:].any() and rebuilt[:, :k].any()


@pytest.mark.parametrize("L", lc.LENS)
@pytest.mark.parametrize("k,m", lc.SOME_CODES)
def test_reconstruct_some_subset_long_shards(codec, oracle, torch, fec, k, m, L):
    """A want mask that names a strict subset of the lost shards: one of two data, one of two parity."""
    c, want = lc.some_subset_case(oracle, k, m, L)
    _, _, st, rebuilt, _ = run_some(codec, fec, torch, c, "interleaved_slack", k, m, L, want=want)
    assert (rebuilt.sum(axis=1) == 2).all() and (rebuilt[:, :k].sum(axis=1) == 1).all() and (st == 0).all()
    assert (c["lost"].sum(axis=1) == 4).all()


# ------------------------------------------------------------------ 3. XOR

@pytest.mark.parametrize("wpc", [6, 0])
@pytest.mark.parametrize("L", lc.LENS)
@pytest.mark.parametrize("k", lc.XOR_KS)
def test_xor_long_shards(codec, oracle, torch, fec, tune, k, L, wpc):
    """xor_encode_kernel and xor_reconstruct_kernel (fec_xor.hip, flat grids), at the shipped residency
    and uncapped: nothing lost, one data shard lost, parity lost, two lost with a data shard among them."""
    tune(xor_wpc=wpc)
    run_xor(codec, fec, torch, lc.xor_case(oracle, k, L), "interleaved_slack", k, L)


# ------------------------------------------------------------------ 4. host-resident forms

def host_buffer(torch, arr, pinned):
    """(what the codec is given, its numpy view): a numpy array (FEC_HOST) or a pinned tensor."""
    if not pinned:
        buf = arr.copy()
        return buf, buf
    t = torch.from_numpy(arr.copy()).pin_memory()
    return t, t.numpy()


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("k,m", lc.HOST_CODES)
def test_host_forms_4375_chunks(codec, oracle, torch, fec, tune, k, m, pinned):
    """FEC_HOST and FEC_HOST_PINNED on packed shards (stride = length) of 69 989 bytes, nine blocks in
    chunks of two (five chunks, the last of one block): encode, then reconstruct over all five mask
    kinds; statuses, return code and every byte of the array."""
    c = lc.host_case(oracle, k, m)
    B = lc.HOST_B
    tune(host_chunk=lc.HOST_CHUNK)
    enc = c["sh"].copy()
    enc[:, k:] = ERASED
    buf, view = host_buffer(torch, enc, pinned)
    codec.rs_encode(k, m, buf)
    assert np.array_equal(view, c["sh"])
    buf, view = host_buffer(torch, c["dmg"], pinned)
    st = np.full(B, 7, dtype=np.int32)
    rc = codec.rs_reconstruct(k, m, buf, c["masks"].copy(), status=st)
    assert c["few"].any() and rc == fec.FEC_ERR_TOO_FEW_SHARDS
    assert np.array_equal(st, np.where(c["few"], fec.FEC_ERR_TOO_FEW_SHARDS, 0))
    assert np.array_equal(view, c["rec"])


def test_wide_host_form_257_chunks(codec, oracle, fec, MUL):
    k, m, L, B = lc.HOST_WIDE
    assert B == lc.WIDE_B
    c = lc.wide_case(oracle, fec, MUL, k, m, L)
    got = np.ascontiguousarray(c["dmg"][:, :, :L])      # packed: stride == shard_len
    st = np.full(B, 99, dtype=np.int32)
    rc = codec.rs_reconstruct_wide(k, m, got, np.ascontiguousarray(c["masks"]), status=st)
    assert rc == fec.FEC_ERR_TOO_FEW_SHARDS
    assert np.array_equal(st, c["st_ref"])
    assert np.array_equal(got, c["ref"][:, :, :L])


# ------------------------------------------------------------------ 5. a batch cut in two launches
# As test_verify_batch_cut_into_two_launches: with both block strides 16, block b is the window
# [16 b, 16 b + 70 000) of one stream per shard, and kMaxItems / 4375 + 1 blocks make two launches, the
# last block alone in the second. Every parity byte of a k = 1 code depends on its own data byte only,
# so overlapping blocks write identical values and the result is the per-byte code of the whole stream.
# Each stream is followed by a canary guard (the shard stride is the stream length plus GUARD).

def cut_streams(rng, nstreams):
    """(image, stream offsets, stream bytes T, shard stride, per_launch, B): nstreams streams after
    stream 0, the data; stream 0 drawn from rng, canary elsewhere."""
    per_launch, B, cps, nchunks = lc.cut_shape()
    T = nchunks * 16
    ss = T + GUARD
    offs = [GUARD + i * ss for i in range(1 + nstreams)]
    img = np.full(offs[-1] + ss, CANARY, dtype=np.uint8)
    img[offs[0]:offs[0] + T] = rng.integers(0, 256, T, dtype=np.uint8)
    return img, offs, T, ss, per_launch, B


def one_shard_encode(oracle, k, m, stream):
    """The oracle's parity [m, T] of the stream taken as one long shard of an RS(1, 1 + m) code, or the
    XOR(1, 1) parity (m = 0)."""
    sh = np.zeros((1, 1 + max(m, 1), stream.size), dtype=np.uint8)
    sh[0, 0] = stream
    if m:
        oracle.rs_encode(1, m, sh)
    else:
        oracle.xor_encode(1, sh)
    return sh[0, 1:]


def test_rs_encode_batch_cut_into_two_launches(codec, oracle, torch, fec):
    """RS(1,3): one data stream, two parity streams; each parity stream is the oracle's encode of the
    data stream as one long shard."""
    img, offs, T, ss, per_launch, B = cut_streams(np.random.default_rng(51), 2)
    model = img.copy()
    par = one_shard_encode(oracle, 1, 2, img[offs[0]:offs[0] + T])
    for j in range(2):
        model[offs[1 + j]:offs[1 + j] + T] = par[j]
    dev = torch.from_numpy(img).cuda()
    p = dev.data_ptr()
    assert fec.lib.fec_rs_encode_batch(codec.handle, 1, 2, lc.CUT_L, B, p + offs[0], 16, p + offs[1], 16, ss,
                                       fec.FEC_DEVICE) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    check_arena(dev.cpu().numpy(), model, "encode cut in two")


def test_xor_encode_batch_cut_into_two_launches(codec, oracle, torch, fec):
    img, offs, T, ss, per_launch, B = cut_streams(np.random.default_rng(52), 1)
    model = img.copy()
    model[offs[1]:offs[1] + T] = one_shard_encode(oracle, 1, 0, img[offs[0]:offs[0] + T])[0]
    dev = torch.from_numpy(img).cuda()
    p = dev.data_ptr()
    assert fec.lib.fec_xor_encode_batch(codec.handle, 1, lc.CUT_L, B, p + offs[0], 16, p + offs[1], 16, ss,
                                        fec.FEC_DEVICE) == fec.FEC_OK
    assert codec.lib_sync_rc() == fec.FEC_OK
    check_arena(dev.cpu().numpy(), model, "xor encode cut in two")


def test_rs_reconstruct_batch_cut_into_two_launches(codec, oracle, torch, fec):
    """RS(1,3) in place with every block's data shard erased: sorted plans + the wave form, cut by the
    item limit through fill_recon_slice, one plan workspace for both launches. Then with one block of
    each launch short of shards: status -4 for those two and the sticky code; their windows are rebuilt
    by their neighbours, but for the stream's last chunk, which belongs to the last block alone."""
    img, offs, T, ss, per_launch, B = cut_streams(np.random.default_rng(53), 2)
    d0 = offs[0]
    par = one_shard_encode(oracle, 1, 2, img[d0:d0 + T])
    for j in range(2):
        img[offs[1 + j]:offs[1 + j] + T] = par[j]
    model = img.copy()                                  # the original data, the parity unchanged
    img[d0:d0 + T] = ERASED
    h = codec.handle
    for what, short in (("all rebuilt", []), ("two blocks short of shards", [per_launch // 3, B - 1])):
        masks = np.full(B, 0b110, dtype=np.uint32)
        masks[short] = 0
        st_want = np.zeros(B, dtype=np.int32)
        st_want[short] = fec.FEC_ERR_TOO_FEW_SHARDS
        want = model.copy()
        if short:
            assert short[0] < per_launch <= short[1] == B - 1
            want[d0 + T - 16:d0 + T] = ERASED
        dev = torch.from_numpy(img).cuda()
        p = dev.data_ptr()
        dm = torch.from_numpy(masks.view(np.int32)).cuda()
        st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
        assert fec.lib.fec_rs_reconstruct_batch(h, 1, 2, lc.CUT_L, B, p + d0, 16, p + offs[1], 16, ss, dm.data_ptr(),
                                                st.data_ptr(), fec.FEC_DEVICE) == fec.FEC_OK
        expect_sync(codec, fec, st_want)
        got = st.cpu().numpy()
        assert np.array_equal(got, st_want), "%s: statuses differ at blocks %s" % (what, np.flatnonzero(got != st_want)[:8])
        check_arena(dev.cpu().numpy(), want, what)
