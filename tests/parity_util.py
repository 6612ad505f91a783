"""What the GPU parity tests share: the tolerance for parity with the reference, the comparison
at that tolerance, the largest relative deviation (for reports) and the valid gm_kernel grids."""
import numpy as np

RTOL = 1e-9
ATOL = 1e-300


def close(got, want, what=""):
    """The GPU tests' comparison with reference values: rtol 1e-9 (FP64, re-associated sums)."""
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=what)


def deviation(got, want):
    """Largest relative deviation over the entries of `want` that are not 0."""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    nz = want != 0
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0


def isolated(pred, gap=1e-7):
    """Every adjacent gap of the sorted predictions is well above the FP64 re-association noise:
    only then is their order, and with it the metrics, set by the algorithm."""
    srt = np.sort(pred)
    gaps = np.diff(srt) / np.maximum(np.abs(srt[1:]), 1e-300)
    return gaps.size == 0 or gaps.min() > gap


def gm_valid_cs(K):
    """GM<K>::cs_ok: workgroups per S part that divide the NQ fixed X groups of QC chunks (up to
    four above K = 16 -- at K >= 25 on plans with fewer parts than CUs, like these -- two at
    K <= 16) and keep one workgroup's S accumulators within 8 chunks (csrc/mmsbm.hip GM)."""
    nch = (K * K + 63) // 64
    qc = (nch + 1) // 2 if K <= 16 else (nch + 3) // 4  # (K >= 25: these small plans take GM::Q4)
    nq = (nch + qc - 1) // qc
    return [cs for cs in range(1, nq + 1) if nq % cs == 0 and (cs > 1 or nch <= 8) and (nq // cs) * qc <= 8]
