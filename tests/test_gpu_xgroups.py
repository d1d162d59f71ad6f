"""GPU: one grouping of the terms by X-part (csrc/xgroups.hip) behind both of its consumers.  Column j of the CSR matrix (kernels.to_csr,
csrc/sparse_matrix.hip) equals H e_j of the matrix-free product (kernels.MatvecPlan, csrc/matvec.hip) under ==, for any finite
coefficients: in row b only the group with x = b ^ j meets the one of e_j, so (H e_j)[b] is D_g(b) * (1 + 0i) plus a +-0 per other group
— D_g(b) itself (the sign of a zero aside) — and the CSR entry (b, j) is the same D_g(b) or, where it is +-0, not stored.  The two agree
exactly when they form the same groups with the same term order inside each one.  tests/test_matvec_oracle.py holds the CPU twin."""
import numpy as np
import pytest

import _sparse_oracle as so
from symmer_amd import kernels, packing
from test_gpu_matvec import family, gaussian

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 8]                                              # 2, 8 and 256 unit vectors per operator
FAMILIES = ['diag1', 'diag130', 'xall', 'distinct', 'random300']


def consumer_cases(n):
    """(family name, bool[T, 2n], Gaussian complex128[T]) of every family on n qubits."""
    for k, name in enumerate(FAMILIES):
        rng = np.random.default_rng(3000 * n + k)
        symp = family(name, n, rng)
        yield name, symp, gaussian(rng, symp.shape[0])


def dense_of_csr(csr, n):
    """complex128[2^n, 2^n] of (data, indices, indptr); what is not stored is 0."""
    data, indices, indptr = csr
    out = np.zeros((1 << n, 1 << n), dtype=np.complex128)
    out[np.repeat(np.arange(1 << n), np.diff(indptr)), indices] = data
    return out


def n_groups(symp, n):
    return len(np.unique(so.bits_to_int(symp[:, :n])))


@pytest.mark.parametrize('n', SIZES)
def test_csr_columns_equal_the_product_with_unit_vectors(n):
    side = 1 << n
    for name, symp, c in consumer_cases(n):
        with kernels.DeviceOp.upload(packing.pack_rows(symp), c) as op:
            A = dense_of_csr(kernels.to_csr(op, n), n)
            with kernels.MatvecPlan(op, n) as plan:
                assert plan.info()[2] == n_groups(symp, n), name
                for j in range(side):
                    e = np.zeros(side, dtype=np.complex128)
                    e[j] = 1.0
                    col, _ = plan.matvec(e)
                    assert np.array_equal(col, A[:, j]), f'{name}: column {j} of the CSR matrix is not H e_{j}'


def test_plan_at_32_qubits():
    """The widest key: 32 sorted bits, the shift by 64 - n = 32; qubit 0, the top bit of the key, set in some terms.  No vector is made."""
    n, rng = 32, np.random.default_rng(32)
    symp = family('random300', n, rng)
    assert 0 < symp[:, 0].sum() < 300 and 0 < symp[:, n - 1].sum() < 300
    G = n_groups(symp, n)
    assert 1 < G < 300                                         # repeated X-parts and distinct ones
    with kernels.DeviceOp.upload(packing.pack_rows(symp), gaussian(rng, 300)) as op, kernels.MatvecPlan(op, n) as plan:
        assert plan.info() == (n, 300, G, 300 * 20 + G * 8 + 4)
