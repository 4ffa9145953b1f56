"""Pure-Python restatement of the monitor from several components (mm-admm_amd/csrc/
kernels/field_math.h: field_accumulate, field_plain_monitor, field_metric_diag): the Hessians, |H|, the
Jacobi, Huang's normalisation and the solve are those of field_monitor_py / field_huang_py; only the
accumulation of the metric, the Jacobi on it and the calls are added.  Scalar loops on Python floats,
so the C++ host function and the device kernels must agree with it bit for bit.

U[v] = [u_0, .., u_{C-1}] per node; w a list of C weights (None: all 1.0)."""
import field_huang_py as hp
import field_monitor_py as fp


def metric(D, Hs, w):
    """A[v] = w_0 |H_0| + w_1 |H_1| + ..., ascending c, from the first product; Hs[c][v] D x D."""
    A = None
    for c, H in enumerate(Hs):
        ab = [fp.abs_sym(D, Hv) for Hv in H]
        if c == 0:
            A = [[[w[0] * a[i][j] for j in range(D)] for i in range(D)] for a in ab]
        else:
            A = [[[Av[i][j] + w[c] * a[i][j] for j in range(D)] for i in range(D)] for Av, a in zip(A, ab)]
    return A


def hessians(D, X, F, U):
    """Hs[c][v]: the scalar recovery of every column."""
    return [fp.hessian(D, X, F, [row[c] for row in U]) for c in range(len(U[0]))]


def monitor(D, X, F, U, w=None, alpha=None, normalise=False, Hs=None):
    """(H, A, M, alpha_used, passes): H[v][c], A[v], M[v] nested D x D lists.  normalise with alpha None:
    solved; M is None when there is no alpha to build it with (plain, alpha None).  Hs: hessians(...)
    of the same arguments, to skip recomputing them."""
    C = len(U[0])
    w = [1.0] * C if w is None else list(w)
    Hs = hessians(D, X, F, U) if Hs is None else Hs
    A = metric(D, Hs, w)
    H = [[Hs[c][v] for c in range(C)] for v in range(len(X))]
    passes = 0
    if not normalise:
        if alpha is None:
            return H, A, None, None, 0
        M = [[[(1.0 if i == j else 0.0) + Av[i][j] / alpha for j in range(D)] for i in range(D)] for Av in A]
        return H, A, M, alpha, 0
    L = [hp.abs_sym_diag(D, Av)[1] for Av in A]  # the Jacobi on A: its diagonal, not its re-assembly
    if alpha is None:
        alpha, passes = hp.solve(D, L, hp.omegas(D, X, F))
    M = []
    for Av, l in zip(A, L):
        t = hp.rho_t(D, l, alpha)[1]
        M.append([[((1.0 if i == j else 0.0) + Av[i][j] / alpha) / t for j in range(D)] for i in range(D)])
    return H, A, M, alpha, passes
