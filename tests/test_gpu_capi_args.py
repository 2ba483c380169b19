"""The argument checks of the 13 batch entry points that need a ctx and a code (fec_hip.h: after
the host-side checks come nblocks == 0, the null pointers, m == 0, then the FEC_DEVICE layout of
each region in order: base and strides 16-byte aligned, then shard_stride >= shard_len; then the
4-byte alignment of the word arrays). One table for all calls: RS(3,2) (XOR(3,1)), one block of
17-byte shards at stride 32. Every case returns before any launch."""
import pytest

from arena import CANARY
from capi_calls import CALLS, layout

pytestmark = pytest.mark.gpu

OK, INV, ALIGN = 0, -1, -7   # FEC_OK, FEC_ERR_INVALID_ARG, FEC_ERR_ALIGNMENT


def expected(call, v):
    """The code fec_hip.h documents for the named values v, or None when every check passes."""
    m = 1 if call.xor else v["m"]
    if v["nblocks"] == 0 or (call.early_m0 and m == 0):
        return OK
    no_parity = m == 0   # (never for the XOR calls) parity may be null and stands for data
    for f in call.need:
        if v[f] is None and not (f == "parity" and no_parity):
            return INV
    for r in call.regions:
        src = "data" if r == "parity" and no_parity else r
        if v[src] % 16 or v[src + "_bs"] % 16 or v["ss"] % 16:
            return ALIGN
        if v["ss"] < v["shard_len"]:
            return INV
    for a, b in call.words:
        if ((v[a] or 0) | ((v[b] or 0) if b else 0)) & 3:
            return ALIGN
    return None


def cases(call):
    """Named-value overrides that trip each check of `call` in turn, and pairs of them."""
    nulls = dict(data=None, parity=None, mask=None, status=None, lens=None, want=None, count=None, out=None)
    out = [dict(nblocks=0, **nulls)]
    if not call.xor:
        out += [dict(m=0, **nulls), dict(m=0, parity=None, data=None), dict(m=0, parity=None, ss=16),
                dict(m=0, parity=None, ss=24), dict(m=0, parity=None, data="+8"), dict(m=0, parity=None, data_bs=40)]
        out += [dict(m=0, parity=None, **{w: "+2"}) for pair in call.words for w in pair if w]
    out += [{f: None} for f in call.need]
    for r in call.regions:
        out += [{r: "+8"}, {r + "_bs": 40}, {r + "_bs": 8}, {r: "+8", "ss": 16}, {r: "+4", "mask": "+2"}]
        out += [{r: "+8", f: None} for f in call.need if f != r]
    out += [dict(ss=24), dict(ss=16), dict(ss=0), dict(ss=16, shard_len=16, data="+1")]
    for a, b in call.words:
        for w in (a, b):
            if w:
                out += [{w: "+2"}, {w: "+1"}, {w: "+2", "ss": 16}, {w: "+2", "ss": 24}, {w: "+2", "data": None}]
    # optional arrays may be null: the check that then fails is the next one
    optional = [w for pair in call.words for w in pair if w and w not in call.need]
    first = call.words[0][0] if call.words else None
    out += [{w: None, first: "+2"} for w in optional if w != first]
    return out


@pytest.mark.parametrize("call", CALLS, ids=lambda c: c.name)
def test_device_argument_checks(call, fec):
    import torch
    assert torch.cuda.is_available(), "GPU test needs a HIP device"
    codec = fec.Codec(0).use_torch_stream()
    try:
        buf = torch.full((1024,), CANARY, dtype=torch.uint8, device="cuda")
        words = torch.full((64,), 99, dtype=torch.int32, device="cuda")
        p, q = buf.data_ptr(), words.data_ptr()
        F = getattr(fec.lib, call.name)
        for mask_words in ((1, 2) if "mask_words" in call.tail else (1,)):
            for over in cases(call):
                v = dict(ctx=codec.handle, k=3, m=2, shard_len=17, nblocks=1, data=p, data_bs=160, parity=p + 96,
                         parity_bs=160, ss=32, mask=q, status=q + 32, lens=q + 64, want=q + 96, count=q + 128,
                         out=p + 256, out_bs=64, out_slots=2, mask_words=mask_words, flags=fec.FEC_DEVICE)
                for f, x in over.items():
                    v[f] = v[f] + int(x) if isinstance(x, str) else x
                want = expected(call, v)
                assert want is not None, ("the case would launch", call.name, over)
                assert F(*layout(call, v)) == want, (call.name, mask_words, over)
        assert codec.lib_sync_rc() == fec.FEC_OK
        assert (buf.cpu() == CANARY).all() and (words.cpu() == 99).all()
    finally:
        codec.close()
