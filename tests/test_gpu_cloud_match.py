"""GPU test of the matcher on clouds that live on the device (clipper_hip_cloud_match: host_cloud.hpp, k_match_select and
k_match_pad in k_match.hip.h) against the host-buffer call clipper_hip_match_descriptors on the same descriptors: the
number of rows, A, sqd and the forward lists, byte for byte. The filters of the one run on the device, of the other on
the host; both read match_rules.hpp. No tolerance anywhere: the statement is an equality of bytes.

Sizes: n0 = 1 (a lone query), 63 / 64 / 65 (the wave edge), 257 (past a workgroup of 256), 1025 (past one chunk of the
1024-wide scan); n1 = 1 (the single-point rule of the ratio test), knn - 1 (fewer points than neighbours asked for;
knn = 1 makes that an empty set, which both routes refuse), 64, 300; d = 1, 32, 33, 64 (one group, four groups unpadded,
FPFH's 33 padded to 40, the widest); knn = 1, 2, 8."""
import numpy as np
import pytest

from clipper_amd import _abi as abi

pytestmark = pytest.mark.gpu

N0 = [1, 63, 64, 65, 257, 1025]
DS = [1, 32, 33, 64]
KNNS = [1, 2, 8]


def _descriptors(rng, d, n, dup):
    """generic: distinct rows, no two distances equal; dup: few distinct values, so rows repeat, distances tie (also at
    0) and the index decides"""
    return np.asfortranarray(rng.integers(0, 3, (d, n)).astype(np.float64) if dup else rng.random((d, n)))


def _cloud(F):
    c = abi.DeviceCloud(np.zeros((3, F.shape[1])))
    return c.set_descriptors(F)


def _same(c0, c1, F0, F1, **kw):
    """both routes on the same inputs: every output equal to the last byte; returns the host's (A, sqd, idx, lsq)"""
    A, sqd, idx, lsq = abi.match_descriptors(F0, F1, return_lists=True, **kw)
    pairs, cidx, clsq = c0.match(c1, return_lists=True, **kw)
    with pairs:
        assert len(pairs) == len(A), (kw, len(pairs), len(A))
        cA, csqd = pairs.download()
    assert cA.dtype == np.int32 and cA.shape == A.shape and cA.tobytes() == A.tobytes(), kw
    assert csqd.tobytes() == sqd.tobytes(), kw
    assert cidx.tobytes() == idx.tobytes() and clsq.tobytes() == lsq.tobytes(), kw
    return A, sqd, idx, lsq


@pytest.mark.parametrize("dup", [False, True], ids=["generic", "ties"])
@pytest.mark.parametrize("n0", N0)
def test_rows_equal_the_host_route(n0, dup):
    rng = np.random.default_rng(1000 * n0 + dup)
    seen_empty = seen_full = seen_bound = 0
    for d in DS:
        F0 = _descriptors(rng, d, n0, dup)
        with _cloud(F0) as c0:
            for n1 in (1, 7, 64, 300):             # 7 = knn - 1 at knn = 8; knn - 1 at knn = 2 is the n1 = 1 above
                F1 = _descriptors(rng, d, n1, dup)
                with _cloud(F1) as c1:
                    for knn in KNNS:
                        for mutual in (False, True):
                            A, sqd, idx, lsq = _same(c0, c1, F0, F1, knn=knn, mutual=mutual)
                            if not mutual and n1 >= knn:         # nothing is filtered: every list entry is a row
                                assert len(A) == n0 * knn
                                seen_full += 1
                            # a bound that lands exactly on one pair's distance: that pair is kept (<=)
                            bound = float(np.sort(lsq[:, 0])[len(lsq) // 2])
                            if bound > 0.0:
                                B, bsqd, _, _ = _same(c0, c1, F0, F1, knn=knn, mutual=mutual, max_sqdist=bound)
                                assert not mutual and (bsqd == bound).any() or mutual
                                seen_bound += 1
                            if knn == 1:                         # Lowe's test; with n1 = 1 the single-point rule
                                R, _, _, _ = _same(c0, c1, F0, F1, knn=1, mutual=mutual, ratio=0.8)
                                if n1 == 1 and not mutual:
                                    assert len(R) == n0
                        if not dup:                              # a bound below every distance: no row at all
                            E, _, _, _ = _same(c0, c1, F0, F1, knn=knn, mutual=False, max_sqdist=1e-300)
                            assert len(E) == 0
                            seen_empty += 1
    assert seen_full and seen_bound and (dup or seen_empty)


def test_an_empty_set_is_refused_by_both_routes():
    F = np.asfortranarray(np.random.default_rng(3).random((33, 5)))
    with pytest.raises(abi.ClipperError, match="error -1: both descriptor sets need at least one point"):
        abi.match_descriptors(F, np.zeros((33, 0), order="F"))
    with abi.DeviceCloud(np.zeros((3, 0))) as empty, _cloud(F) as c:
        with pytest.raises(abi.ClipperError, match="error -1: .*the cloud has no points"):
            empty.set_descriptors(np.zeros((33, 0), order="F"))
        with pytest.raises(abi.ClipperError, match="error -5: .*has no descriptors"):     # CLIPPER_HIP_E_STATE
            c.match(empty)


def test_refusals_and_states():
    rng = np.random.default_rng(4)
    F = np.asfortranarray(rng.random((32, 20)))
    with _cloud(F) as c0, _cloud(np.asfortranarray(rng.random((33, 20)))) as c1, abi.DeviceCloud(np.zeros((3, 20))) as bare:
        with pytest.raises(abi.ClipperError, match="error -1: .*descriptors of 32 and 33 coordinates"):
            c0.match(c1)
        with pytest.raises(abi.ClipperError, match="error -5: .*has no descriptors"):
            c0.match(bare)
        with pytest.raises(abi.ClipperError, match="error -5: .*never computed"):
            bare.descriptors()
        for kw, msg in ((dict(knn=9), "knn must be in 1..8"), (dict(knn=2, ratio=0.8), "the ratio test needs knn == 1"),
                        (dict(ratio=1.5), "ratio must be 0")):
            with pytest.raises(abi.ClipperError, match="error -1: .*" + msg):
                c0.match(c0, **kw)
        bad = F.copy(order="F")
        bad[5, 7] = np.inf
        with pytest.raises(abi.ClipperError, match="F: non-finite value at coordinate 5 of descriptor 7"):
            bare.set_descriptors(bad)
        assert c0.descriptors().tobytes() == F.tobytes()        # what went up comes down
        A, sqd = c0.match(c0).download()                        # and the cloud is still usable: every point finds itself
        assert np.array_equal(A, np.stack([np.arange(20)] * 2, axis=1)) and not sqd.any()


def test_pairs_round_trip():
    A = np.array([[0, 5], [3, 1], [2, 2]], dtype=np.int32)
    sqd = np.array([0.5, 0.25, 0.0])
    with abi.DevicePairs(A, sqd) as p:
        assert len(p) == 3
        gA, gs = p.download()
        assert np.array_equal(gA, A) and np.array_equal(gs, sqd)
    with abi.DevicePairs(A) as p:
        assert np.array_equal(p.download(), A)
        with pytest.raises(abi.ClipperError, match="error -5: .*no squared distances"):
            p.download(with_sqd=True)
    with abi.DevicePairs() as p:
        assert len(p) == 0 and p.download().shape == (0, 2)
