"""The scheme layer over codes of more than 32 shards: NewReedSolomonScheme(k, m) recovers whatever
it encodes (reed_solomon.go:15-23, :92-136), through the wide reconstruct call."""
import numpy as np
import pytest

from scheme_util import scheme_mod

pytestmark = pytest.mark.gpu

LENS = [1, 33, 700, 1200]
FIRST = 20   # smallest SSID of the block


@pytest.fixture(scope="module")
def S(fec):
    import torch
    assert torch.cuda.is_available()
    return scheme_mod()


def _block(S, k, m, payloads, sources, repairs):
    return S.Block.literal(id=1, tot_src=k, tot_rep=m, biggest=max(len(p) for p in payloads), smallest=FIRST,
                           largest=FIRST + k - 1, sources={FIRST + i: (payloads[i], 1452) for i in sources},
                           repairs=repairs)


@pytest.mark.parametrize("k,m", [(40, 10), (100, 50)])
def test_wide_scheme_recovers_dropped_sources(S, k, m):
    rng = np.random.default_rng(k + m)
    s, err = S.new_reed_solomon_scheme(k, m)
    assert err is None
    payloads = [bytes(rng.integers(0, 256, LENS[i % len(LENS)], dtype=np.uint8)) for i in range(k)]
    frames, err = s.repair_symbols(_block(S, k, m, payloads, range(k), {}))
    assert err is None and len(frames) == m and [f[1] for f in frames] == list(range(m))
    assert all(len(f[2]) == max(LENS) + 2 for f in frames)
    nlost = min(m, 7)
    # sources around the mask word boundary among the dropped ones
    rest = [i for i in rng.permutation(k).tolist() if i not in (31, 32)]
    lost = sorted([31, 32] + rest[:nlost - 2])
    kept = [i for i in range(k) if i not in lost]
    # drop some repairs too: keep exactly as many as sources were lost, not the first ones
    keep_rep = sorted(rng.choice(m, size=len(lost), replace=False).tolist())
    repairs = {pid: frames[pid][2] for pid in keep_rep}
    got, err = s.recover_symbol_payloads(_block(S, k, m, payloads, kept, repairs))
    assert err is None
    # the dropped payloads in ascending order, each cut to its length trailer (reed_solomon.go:128-133)
    assert got == b"".join(payloads[i] for i in lost)
    # one repair fewer: fewer than k symbols
    repairs.pop(keep_rep[0])
    got, err = s.recover_symbol_payloads(_block(S, k, m, payloads, kept, repairs))
    assert got is None and err == "not enough present symbols to repair the missing ones"
    # nothing lost: nil, nil
    got, err = s.recover_symbol_payloads(_block(S, k, m, payloads, range(k), {}))
    assert (got, err) == (None, None)
