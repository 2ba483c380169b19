"""The 13 batch entry points of include/fec_hip.h as one table, for the tests that pin their
argument checks (test_capi_exports.py without a device, test_gpu_capi_args.py with one): each
call's limits as the header documents them and its argument list by field name, so one set of
named values can be laid out as any call's positional arguments."""
from collections import namedtuple

# max_n: largest k + m; host: FEC_HOST / FEC_HOST_PINNED accepted; early_m0: m == 0 returns FEC_OK
# before the pointers are looked at (the encodes); need: pointers that must not be null (parity only
# while m > 0, except for the XOR calls, which have no m); regions: what check_device_layout sees,
# in order; words: the (array, array) pairs of check_device_words, in order; tail: the arguments
# between shard_stride and flags.
Call = namedtuple("Call", "name max_n host early_m0 need regions words tail xor")

_RECON = ("data", "mask", "parity")
CALLS = [
    Call("fec_rs_encode_batch", 256, True, True, ("data", "parity"), ("data", "parity"), (), (), False),
    Call("fec_rs_reconstruct_batch", 32, True, False, _RECON, ("data", "parity"), (("mask", "status"),),
         ("mask", "status"), False),
    Call("fec_rs_recover_batch", 32, False, False, _RECON + ("out",), ("data", "parity", "out"),
         (("mask", "status"),), ("mask", "out", "out_bs", "out_slots", "status"), False),
    Call("fec_rs_reconstruct_wide_batch", 256, True, False, _RECON, ("data", "parity"), (("mask", "status"),),
         ("mask", "mask_words", "status"), False),
    Call("fec_rs_recover_wide_batch", 256, False, False, _RECON + ("out",), ("data", "parity", "out"),
         (("mask", "status"),), ("mask", "mask_words", "out", "out_bs", "out_slots", "status"), False),
    Call("fec_rs_encode_ragged_batch", 256, False, True, ("data", "parity", "lens"), ("data", "parity"),
         (("lens", "status"),), ("lens", "status"), False),
    Call("fec_rs_reconstruct_ragged_batch", 32, False, False, _RECON + ("lens",), ("data", "parity"),
         (("mask", "status"), ("lens", None)), ("mask", "lens", "status"), False),
    Call("fec_rs_recover_ragged_batch", 32, False, False, _RECON + ("lens", "out"), ("data", "parity", "out"),
         (("mask", "status"), ("lens", None)), ("mask", "lens", "out", "out_bs", "out_slots", "status"), False),
    Call("fec_rs_verify_batch", 256, False, False, ("data", "status", "parity"), ("data", "parity"),
         (("count", "status"),), ("status", "count"), False),
    Call("fec_rs_reconstruct_some_batch", 32, False, False, _RECON, ("data", "parity"),
         (("mask", "status"), ("want", None)), ("mask", "want", "status"), False),
    Call("fec_xor_encode_batch", 256, True, False, ("data", "parity"), ("data", "parity"), (), (), True),
    Call("fec_xor_reconstruct_batch", 32, True, False, ("data", "parity", "mask"), ("data", "parity"),
         (("mask", "status"),), ("mask", "status"), True),
]


def layout(call, v):
    """The positional arguments of `call` from the named values v (ctx first, flags last)."""
    head = [v["ctx"], v["k"]] + ([] if call.xor else [v["m"]])
    body = [v["shard_len"], v["nblocks"], v["data"], v["data_bs"], v["parity"], v["parity_bs"], v["ss"]]
    return tuple(head + body + [v[f] for f in call.tail] + [v["flags"]])
