"""What tests/test_hip_isq.py leans on, proven without a GPU: the main case clips at both ends, decoding changes the matrix,
and at every width with d >= 8 another summation order over the DECODED rows changes a compared distance."""
import numpy as np
import pytest

from tests import isq_cases as S
from tests import ivf_cases as C
from tests import width_cases as W

SQ8_WIDTHS = list(W.WIDTHS) + [8193, 8199, 8200]


def test_main_case_clips_and_decoding_changes_the_rows():
    case = C.make_case(36)
    sc = S.make(case, S.SQ_ISQ_SQ8)
    x = case.x
    assert ((sc.codes == 0) & (x < sc.vmin)).any(), "no code 0 produced by clipping"
    assert ((sc.codes == 255) & (x > sc.vmin + sc.step * np.float32(255))).any(), "no code 255 produced by clipping"
    for kind in S.KINDS.values():
        dec = S.make(case, kind).dec.x
        assert dec.dtype == np.float32 and dec.shape == x.shape and (dec != x).any()
    assert np.array_equal(S.decode(S.encode(x, S.SQ_ISQ_F16), S.SQ_ISQ_F16), x.astype(np.float16).astype(np.float32))


@pytest.mark.parametrize("kind,d", [("sq8", d) for d in SQ8_WIDTHS if d >= 8] + [("f16", d) for d in S.F16_WIDTHS if d >= 8])
def test_another_order_over_the_decoded_rows_changes_a_distance(kind, d):
    seq, _ = C.orders_that_differ(S.make(C.make_width_case(d), S.KINDS[kind]).dec)
    assert seq > 0, f"{kind} d={d}: a left-to-right sum gives numpy's bits in all 50 distances"
