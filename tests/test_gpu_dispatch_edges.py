"""Kernel instances and dispatch boundaries of the decode and encode launches that no benchmark
code reaches, bit-exact against the CPU oracle, in the compact split layout ([B][k][S] data,
[B][m][S] parity, S = round_up(L, 16)):

* the routed in-place kernel (fec_recover.hip routed_recon_applies: every k = 8, 2 <= m <= 8 code)
  on m = 2, 3 and 8 -- m = 8 sits on both of its limits (128 coefficient words, a 16 KiB PermTab
  table) and is the only user of the MAXE = 8 instances;
* the direct single-erasure body picked by k alone (launch_rs_recover_direct): the compile-time
  k = 8 / 16 / 20 bodies with m they were not written for, the runtime-k body with 2-3 input
  groups and an odd tail, rows from the kernel argument and from the PermTab table on both sides
  of the argument's size limit;
* the `cps < 32` gate shared by the direct and the wave forms, at 31 and 32 chunks per shard;
* encodes wider than any decodable code: parity rows in passes of 16, the 64 KiB LDS table and
  the tables read from global memory (m * k > 2048 per pass).

Every array the library may write is compared whole: a rebuilt or encoded shard is its bytes
[0, L) and zeros up to S, everything else is as it was before the call.
"""
import numpy as np
import pytest

from arena import codec, rup16, torch  # noqa: F401

pytestmark = pytest.mark.gpu

FILL_ERASED = 0x3C
FILL_OUT = 0xEE


def make_batch(oracle, rng, k, m, L, B):
    """Encoded shards [B, k + m, S], zero from L to S (so the oracle's full-S results carry the
    zero padding the kernels write)."""
    sh = np.zeros((B, k + m, rup16(L)), dtype=np.uint8)
    sh[:, :k, :L] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
    return oracle.rs_encode(k, m, sh)


def lost_of(masks, n):
    return ((masks[:, None] >> np.arange(n)[None, :]) & 1) == 0


def random_masks(rng, B, k, m, max_loss):
    n = k + m
    masks = np.empty(B, dtype=np.uint32)
    for b in range(B):
        lost = rng.choice(n, size=int(rng.integers(0, max_loss + 1)), replace=False)
        masks[b] = ((1 << n) - 1) & ~int(sum(1 << int(i) for i in lost))
    return masks


def oracle_inplace(oracle, k, m, sh, masks):
    """(damaged batch, the oracle's in-place reconstruct of it, its statuses as the ABI reports
    them: 0 or FEC_ERR_TOO_FEW_SHARDS)."""
    dmg = sh.copy()
    dmg[lost_of(masks, k + m)] = FILL_ERASED
    rec = dmg.copy()
    st = oracle.rs_reconstruct(k, m, rec, masks)
    return dmg, rec, np.where(st != 0, -4, 0)


def sync_code(fec, st_want):
    return (fec.FEC_ERR_TOO_FEW_SHARDS if (st_want == fec.FEC_ERR_TOO_FEW_SHARDS).any() else
            fec.FEC_ERR_INVALID_ARG if (st_want == fec.FEC_ERR_INVALID_ARG).any() else fec.FEC_OK)


def check_inplace(codec, oracle, torch, fec, k, m, L, sh, masks):
    B = sh.shape[0]
    dmg, rec, st_want = oracle_inplace(oracle, k, m, sh, masks)
    ok = st_want == 0
    assert np.array_equal(rec[ok][:, :k], sh[ok][:, :k])         # the oracle gives back the data
    d = torch.from_numpy(np.ascontiguousarray(dmg[:, :k])).cuda()
    par = torch.from_numpy(np.ascontiguousarray(dmg[:, k:])).cuda()
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_reconstruct_split(k, m, d, par, torch.from_numpy(masks.view(np.int32)).cuda(), status=st, shard_len=L)
    assert codec.lib_sync_rc() == sync_code(fec, st_want)
    assert np.array_equal(st.cpu().numpy(), st_want)
    assert np.array_equal(d.cpu().numpy(), rec[:, :k])           # rebuilt, failed and present shards alike
    assert np.array_equal(par.cpu().numpy(), dmg[:, k:])         # parity only read


def check_recover(codec, oracle, torch, fec, k, m, L, sh, masks, slots):
    B, S = sh.shape[0], sh.shape[2]
    dmg, rec, st_inplace = oracle_inplace(oracle, k, m, sh, masks)
    lost_d = lost_of(masks, k + m)[:, :k]
    e_d = lost_d.sum(axis=1)
    few = (st_inplace != 0)
    assert not (few & (e_d == 0)).any()
    st_want = np.where(e_d == 0, 0, np.where(few, fec.FEC_ERR_TOO_FEW_SHARDS,
                                             np.where(e_d > slots, fec.FEC_ERR_INVALID_ARG, e_d)))
    want = np.full((B, slots, S), FILL_OUT, dtype=np.uint8)
    for b in np.flatnonzero(st_want > 0):
        miss = np.flatnonzero(lost_d[b])
        want[b, :len(miss)] = rec[b, miss]                       # bytes [0, L), zeros to S
    d = torch.from_numpy(np.ascontiguousarray(dmg[:, :k])).cuda()
    par = torch.from_numpy(np.ascontiguousarray(dmg[:, k:])).cuda()
    out = torch.full((B, slots, S), FILL_OUT, dtype=torch.uint8, device="cuda")
    st = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    codec.rs_recover_split(k, m, d, par, torch.from_numpy(masks.view(np.int32)).cuda(), out, status=st, shard_len=L)
    assert codec.lib_sync_rc() == sync_code(fec, st_want)
    assert np.array_equal(st.cpu().numpy(), st_want)
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(d.cpu().numpy(), dmg[:, :k]) and np.array_equal(par.cpu().numpy(), dmg[:, k:])
    return st_want


# ---------------------------------------------------------------- routed in place
# RS(8,10), RS(8,11), RS(8,16) (k = 8, m = 2, 3, 8) and RS(8,12) as the control: single-erasure-only
# batches (the route word stays zero: the direct body <8, 1, 0, WW>) and mixed ones (the wave
# rebuild of the sorted plans, MAXE = 4 for m <= 4, MAXE = 8 for m = 8), on both sides of the
# classify pass's 256-block sweep, on the default route (three working waves), with all four waves
# (route_ww 4) and on the sorted-plan route (dec_route 0).
ROUTE_FORMS = {"routed": dict(dec_route=1), "routed_ww4": dict(dec_route=1, route_ww=4), "plans": dict(dec_route=0)}


@pytest.mark.parametrize("route", sorted(ROUTE_FORMS))
@pytest.mark.parametrize("multi", [False, True])
@pytest.mark.parametrize("B", [63, 257])
@pytest.mark.parametrize("m", [2, 3, 8, 4])
def test_rs_inplace_routed_k8_codes_match_oracle(codec, oracle, torch, fec, tune, m, B, multi, route):
    k, L = 8, 1202
    n = k + m
    rng = np.random.default_rng(1000 * m + 7 * B + int(multi) + 10 * sorted(ROUTE_FORMS).index(route))
    sh = make_batch(oracle, rng, k, m, L, B)
    masks = np.empty(B, dtype=np.uint32)
    for b in range(B):
        kind = int(rng.integers(0, 5))
        if kind == 0:
            lost = []                                                      # intact
        elif kind == 1:
            lost = [int(rng.integers(k, n))]                               # one parity shard
        elif kind == 2 or (kind == 3 and not multi):
            lost = [int(rng.integers(0, k))]                               # one data shard
        elif kind == 3:
            lost = list(rng.choice(n, size=int(rng.integers(2, m + 1)), replace=False))   # up to m shards
        else:
            lost = list(rng.choice(n, size=m + 1, replace=False))          # too few shards (data among them)
        masks[b] = ((1 << n) - 1) & ~sum(1 << int(i) for i in lost)
    masks[B // 3] = ((1 << n) - 1) & ~(1 << 5)                             # one data shard, every parity present
    masks[B // 4] = ((1 << n) - 1) & ~((1 << (m + 1)) - 1)                 # shards 0..m: too few
    if multi:   # a block with min(k, m) erased data shards: every row of the code's largest plan
        masks[B // 2] = ((1 << n) - 1) & ~((1 << min(k, m)) - 1)
    lost = lost_of(masks, n)
    e_d = lost[:, :k].sum(axis=1)
    enough = (n - lost.sum(axis=1)) >= k
    if multi:
        assert (e_d[enough] == min(k, m)).any()
    else:
        assert e_d[enough].max() == 1     # nothing for the plan route: the route word stays zero
    assert (~enough & (e_d > 0)).any()
    tune(**ROUTE_FORMS[route])
    check_inplace(codec, oracle, torch, fec, k, m, L, sh, masks)


# ---------------------------------------------------------------- direct body
# launch_rs_recover_direct picks its kernel by k alone. Single-slot recovers of: (8,1), (8,2),
# (8,8): direct_launch<8,1,3> / <8,0> with m != 4; (16,1), (16,2), (20,1): <16,2> / <20,2> with the
# small codes' tables; (9,1), (13,1): the runtime-k body with two input groups and an odd tail;
# (21,1): three groups, 126 coefficient words (rows from the kernel argument under dec_direct 1);
# (22,1): 132 words, rows from the PermTab table (15 488 bytes, under the 16 KiB cap) either way;
# (6,2): the reference's own RS(6,2) with one slot; (3,2). dec_direct 2: rows from the table for
# every runtime-k and k = 8 code. The m = 1 codes also in place (the direct kernel, nt stores).
DIRECT_CODES = [(8, 1), (8, 2), (8, 8), (9, 1), (13, 1), (21, 1), (22, 1), (16, 1), (16, 2), (20, 1), (6, 2), (3, 2)]


@pytest.mark.parametrize("dec_direct", [1, 2])
@pytest.mark.parametrize("L", [513, 1202])
@pytest.mark.parametrize("k,m", DIRECT_CODES)
def test_rs_direct_body_by_k_matches_oracle(codec, oracle, torch, fec, tune, k, m, L, dec_direct):
    B = 131
    rng = np.random.default_rng(10000 * k + 100 * m + L + dec_direct)
    sh = make_batch(oracle, rng, k, m, L, B)
    masks = random_masks(rng, B, k, m, max_loss=m + 1)
    masks[1] = ((1 << (k + m)) - 1) & ~(1 << (k - 1))           # the last data shard alone
    masks[2] = ((1 << (k + m)) - 1) & ~1                        # the first
    masks[3] = (1 << (k + m)) - 1
    masks[4] = ((1 << (k + m)) - 1) & ~((1 << (m + 1)) - 1)     # shards 0..m lost: too few
    if m >= 2:
        masks[5] = ((1 << (k + m)) - 1) & ~0b11                 # two data shards for one slot
    tune(dec_direct=dec_direct)
    st = check_recover(codec, oracle, torch, fec, k, m, L, sh, masks, slots=1)
    assert (st == 1).any() and (st == 0).any() and (st == fec.FEC_ERR_TOO_FEW_SHARDS).any()
    assert m == 1 or (st == fec.FEC_ERR_INVALID_ARG).any()
    if m == 1:
        check_inplace(codec, oracle, torch, fec, k, m, L, sh, masks)


# ---------------------------------------------------------------- the cps gate
# direct_recon_applies and wave_recon_applies both need 32 chunks per shard: L = 496 (31 chunks:
# plans in block order and the workgroup-tile rebuild for every call), L = 497 and 512 (32 chunks:
# the direct kernels for single-slot recovers and RS(2,3), the routed kernel for RS(8,12) in place,
# sorted plans and the wave rebuild for the rest; a wave's 64 items are exactly two blocks).
@pytest.mark.parametrize("call", ["inplace", "recover_1", "recover_m"])
@pytest.mark.parametrize("L", [496, 497, 512])
@pytest.mark.parametrize("k,m", [(8, 4), (2, 1), (16, 8)])
def test_rs_decode_at_the_chunk_count_gate_matches_oracle(codec, oracle, torch, fec, k, m, L, call):
    B = 131
    rng = np.random.default_rng(100 * k + L)
    sh = make_batch(oracle, rng, k, m, L, B)
    masks = random_masks(rng, B, k, m, max_loss=m + 1)
    masks[5] = ((1 << (k + m)) - 1) & ~(1 << (k - 1))
    masks[6] = ((1 << (k + m)) - 1) & ~((1 << min(k, m)) - 1)   # min(k, m) data shards lost
    masks[7] = ((1 << (k + m)) - 1) & ~((1 << (m + 1)) - 1)     # shards 0..m lost: too few
    if call == "inplace":
        check_inplace(codec, oracle, torch, fec, k, m, L, sh, masks)
    else:
        slots = 1 if call == "recover_1" else m
        st = check_recover(codec, oracle, torch, fec, k, m, L, sh, masks, slots)
        assert (st == 1).any() and (st == fec.FEC_ERR_TOO_FEW_SHARDS).any()
        assert (st == (fec.FEC_ERR_INVALID_ARG if slots < min(k, m) else min(k, m))).any()


# ---------------------------------------------------------------- wide encode
# Encode accepts k + m <= 256 and runs parity rows in passes of 16: (32,32) two passes, (64,64)
# four, (1,255) sixteen (the last of 15 rows); (128,16): m * k = 2048 per pass, the whole 64 KiB LDS
# table; (129,16), (200,56): past it, rs_encode_kernel<16, false> / <8, false> with the tables read
# from global memory; (255,1): the widest data. A parity byte depends on its own column only, so
# one oracle encode per code (37 blocks of 1202 bytes) serves every (B, L) case as a slice.
WIDE_CODES = [(32, 32), (64, 64), (128, 16), (129, 16), (200, 56), (255, 1), (1, 255)]
WIDE_B, WIDE_L = 37, 1202
_wide = {}


def wide_ref(oracle, k, m):
    if (k, m) not in _wide:
        rng = np.random.default_rng(1000 * k + m)
        sh = np.zeros((WIDE_B, k + m, WIDE_L), dtype=np.uint8)
        sh[:, :k] = rng.integers(0, 256, (WIDE_B, k, WIDE_L), dtype=np.uint8)
        oracle.rs_encode(k, m, sh)
        sh.setflags(write=False)
        _wide[(k, m)] = sh
    return _wide[(k, m)]


@pytest.mark.parametrize("L", [17, WIDE_L])
@pytest.mark.parametrize("B", [1, WIDE_B])
@pytest.mark.parametrize("k,m", WIDE_CODES)
def test_rs_wide_encode_matches_oracle(codec, oracle, torch, k, m, B, L):
    ref = wide_ref(oracle, k, m)
    S = rup16(L)
    data = np.zeros((B, k, S), dtype=np.uint8)
    data[:, :, :L] = ref[:B, :k, :L]
    want = np.zeros((B, m, S), dtype=np.uint8)
    want[:, :, :L] = ref[:B, k:, :L]
    d = torch.from_numpy(data).cuda()
    p = torch.full((B, m, S), 0xA5, dtype=torch.uint8, device="cuda")
    codec.rs_encode_split(k, m, d, p, shard_len=L)
    codec.sync()
    assert np.array_equal(p.cpu().numpy(), want)
    assert np.array_equal(d.cpu().numpy(), data)
