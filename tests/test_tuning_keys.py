"""The tuning knobs are declared once, in the library (fec_kernels.hpp FEC_TUNING_KNOBS); the Python
face reads names and keys from it through fec__tuning_name(). tools/go_batch_bench.c and recorded
tool runs pass keys by number, so the nineteen keys in use are pinned here as a literal. No GPU."""
import ctypes

TUNING_KEYS = {"enc_wpc": 0, "gen_wpc": 1, "dec_wpc": 2, "dir_wpc": 3, "enc_bwpc": 4, "enc_fixed": 5,
               "dec_wave": 6, "dec_direct": 7, "host_chunk": 8, "host_threads": 9, "bat_zc": 10,
               "dec_route": 11, "st_pol": 12, "dst_pol": 13, "route_wpc": 14, "route_ww": 15,
               "xor_wpc": 16, "enc_ww": 17, "rag_g": 18}


def test_tuning_keys_are_the_librarys_list(fec):
    assert fec.Codec.TUNING_KEYS == TUNING_KEYS
    assert list(fec.Codec.TUNING_KEYS) == sorted(TUNING_KEYS, key=TUNING_KEYS.get)   # in key order
    name = fec.lib.fec__tuning_name
    for knob, key in TUNING_KEYS.items():
        assert name(key) == knob.encode()
    assert name(19) is None and name(-1) is None


def test_unknown_tuning_key_is_invalid_arg(fec):
    # the key is checked before the ctx is used: any non-null pointer stands in for one here
    stand_in = ctypes.create_string_buffer(8)
    for key in (19, -1):
        assert fec.lib.fec__set_tuning(ctypes.addressof(stand_in), key, 1) == fec.FEC_ERR_INVALID_ARG
    assert fec.lib.fec__set_tuning(None, 0, 1) == fec.FEC_ERR_INVALID_ARG
