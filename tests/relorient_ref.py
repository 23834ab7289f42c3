"""NumPy restatement of photogrammetry/essmat5.m and camsfrome.m (with pm_forwintersect3.m and ptdepth.m, which
camsfrome calls) and a Sampson-count RANSAC over given minimal samples.  Shares no code with dbat_amd/: the tests
measure the device against it.

essmat5 here: the null space from the SVD (essmat5.m:23-24), the ten cubic constraints det E = 0 and
2 E E' E - tr(E E') E = 0 expanded by polynomial products over E = x E1 + y E2 + z E3 + E4 (the products are index
tensors built from exponent arithmetic below; essmat5.m keeps the expanded result as tables), the elimination
A(:,1:10) \\ A(:,11:20) (:27), the action matrix of multiplication by x on the monomials [x^2 xy xz y^2 yz z^2 x y z 1]
(:28-33), its eigenvectors (:35-39) and the reality test of :42.

Layout: a solution e (9) satisfies sum e[a + 3 b] Q1[a] Q2[b] = 0 (essmat5.m:12-20).  camsfrome expects xp' E x = 0:
E = e.reshape(3, 3) with x = Q1, xp = Q2."""
import itertools

import numpy as np

LIN = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
QUAD = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
# graded lexicographic: the ten cubic monomials first (they are eliminated), then the basis of the quotient ring
CUB = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)] + QUAD


def _add(a, b):
    return tuple(i + j for i, j in zip(a, b))


K11 = np.zeros((10, 4, 4))          # quadratic[q] = sum K11[q, i, j] a[i] b[j]
for _i, _j in itertools.product(range(4), range(4)):
    K11[QUAD.index(_add(LIN[_i], LIN[_j])), _i, _j] = 1
K21 = np.zeros((20, 10, 4))         # cubic[c] = sum K21[c, q, l] a[q] b[l]
for _q, _l in itertools.product(range(10), range(4)):
    K21[CUB.index(_add(QUAD[_q], LIN[_l])), _q, _l] = 1


def mul11(a, b):
    return np.einsum('qij,i,j->q', K11, a, b)


def mul21(a, b):
    return np.einsum('cql,q,l->c', K21, a, b)


def design(Q1, Q2):
    """essmat5.m:12-20: row i holds Q1[a, i] Q2[b, i] at column a + 3 b."""
    return np.stack([Q1[a] * Q2[b] for b in range(3) for a in range(3)], 1)


def constraints(EE):
    """The 10 x 20 coefficient matrix over CUB of det E and 2 E E' E - tr(E E') E for E = sum EE[:, m] (x, y, z, 1)[m]."""
    P = [[EE[r + 3 * c] for c in range(3)] for r in range(3)]       # P[r][c]: the linear form of E(r, c)
    rows = []
    det = np.zeros(20)
    for c in range(3):
        c1, c2 = (c + 1) % 3, (c + 2) % 3
        det += mul21(mul11(P[1][c1], P[2][c2]) - mul11(P[1][c2], P[2][c1]), P[0][c])
    rows.append(det)
    S = [[sum(mul11(P[r][c], P[s][c]) for c in range(3)) for s in range(3)] for r in range(3)]     # E E'
    tr = S[0][0] + S[1][1] + S[2][2]
    for r in range(3):
        for c in range(3):
            rows.append(2 * sum(mul21(S[r][s], P[s][c]) for s in range(3)) - mul21(tr, P[r][c]))
    return np.array(rows)


def essmat5(Q1, Q2, imag_tol=0.01, full=False):
    """essmat5.m: 9 x k real solutions.  full: also the ratio |imag(lambda)| / max |lambda| of each one kept."""
    Q1, Q2 = np.asarray(Q1, float), np.asarray(Q2, float)
    V = np.linalg.svd(design(Q1, Q2))[2].T
    EE = V[:, 5:9]
    A = constraints(EE)
    C = np.linalg.solve(A[:, :10], A[:, 10:])
    M = np.zeros((10, 10))
    M[:6] = -C[[0, 1, 2, 3, 4, 5]]          # x times x^2, xy, xz, y^2, yz, z^2: the first six cubic monomials
    M[6, 0] = M[7, 1] = M[8, 2] = M[9, 6] = 1          # x times x, y, z, 1
    lam, W = np.linalg.eig(M)
    sols = W[6:9] / W[9]
    Evec = EE @ np.vstack([sols, np.ones((1, 10))])
    Evec = Evec / np.sqrt(np.sum(Evec ** 2, 0))
    ratio = np.abs(lam.imag) / np.max(np.abs(lam))
    keep = ratio < imag_tol
    out = np.real(Evec[:, keep])
    return (out, ratio[keep]) if full else out


def null_vector(P):
    return np.linalg.svd(P)[2][-1]


def forwintersect3(P, xy):
    """pm_forwintersect3.m:11-73.  P: list of 3 x 4; xy: (2, N, K).  Returns 3 x K."""
    n, k = len(P), xy.shape[2]
    Cc = np.zeros((3, n))
    t = np.zeros((3, k, n))
    for i in range(n):
        nv = null_vector(P[i])
        Cc[:, i] = nv[:3] / nv[3]
        Ppx = np.linalg.pinv(P[i]) @ np.vstack([xy[:, i, :], np.ones((1, k))])
        far = np.abs(Ppx[3]) < 1e-8
        Ppx[:, far] += np.append(Cc[:, i], 1.0)[:, None]
        d = Ppx[:3] / Ppx[3] - Cc[:, i:i + 1]
        t[:, :, i] = d / np.sqrt(np.sum(d * d, 0))
    OP = np.full((3, k), np.nan)
    b = Cc.T.reshape(-1)
    for j in range(k):
        A = np.zeros((3 * n, 3 + n))
        for i in range(n):
            A[3 * i:3 * i + 3, :3] = np.eye(3)
            A[3 * i:3 * i + 3, 3 + i] = t[:, j, i]
        OP[:, j] = np.linalg.lstsq(A, b, rcond=None)[0][:3]
    return OP


def ptdepth(P, X):
    """ptdepth.m:14 for Euclidean X (3 x n)."""
    M = P[:, :3]
    x = P @ np.vstack([X, np.ones((1, X.shape[1]))])
    return np.sign(np.linalg.det(M)) * x[2] / np.linalg.norm(M[2])


def camsfrome(E, x, xp, frontDir):
    """camsfrome.m:16-59: (P1, P2, X (3 x n, in the frame of P1), inFront, sp).  x, xp: 3 x n, last row 1."""
    U, _, Vt = np.linalg.svd(E)
    V = Vt.T
    if np.linalg.det(U) < 0:
        U[:, 2] = -U[:, 2]
    if np.linalg.det(V) < 0:
        V[:, 2] = -V[:, 2]
    W = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])
    P1 = np.eye(3, 4)
    u3 = U[:, 2:3]
    C2 = [np.hstack([U @ W @ V.T, u3]), np.hstack([U @ W @ V.T, -u3]), np.hstack([U @ W.T @ V.T, u3]), np.hstack([U @ W.T @ V.T, -u3])]
    xy = np.stack([x[:2] / x[2], xp[:2] / xp[2]], 1)
    XX, zp = [], np.zeros((4, x.shape[1]), bool)
    for j in range(4):
        X = forwintersect3([P1, C2[j]], xy)
        d1, d2 = ptdepth(P1, X), ptdepth(C2[j], X)
        zp[j] = (np.sign(d1) == np.sign(frontDir)) & (np.sign(d2) == np.sign(frontDir))
        XX.append(X)
    cnt = zp.sum(1)
    ii = np.argsort(-cnt, kind='stable')
    return P1, C2[ii[0]], XX[ii[0]], zp[ii[0]], cnt[ii]


def sampson2(e, x1, x2):
    """Squared Sampson distance of the correspondences x1, x2 (2 x n) under e (sum e[a + 3 b] q1[a] q2[b] = 0)."""
    M = np.asarray(e, float).reshape(3, 3).T                    # M[a, b] = e[a + 3 b]
    q1 = np.vstack([x1, np.ones((1, x1.shape[1]))])
    q2 = np.vstack([x2, np.ones((1, x2.shape[1]))])
    a, b = M @ q2, M.T @ q1
    r = np.sum(q1 * a, 0)
    return r * r / (a[0] ** 2 + a[1] ** 2 + b[0] ** 2 + b[1] ** 2)


def ransac(x1, x2, samples, thr2):
    """The model with the most correspondences below thr2 among the solutions of every sample (rows of five indices);
    ties go to the earliest (sample, solution).  dict(e, count, mask, sample, sol, models)."""
    best = dict(e=np.full(9, np.nan), count=0, mask=np.zeros(x1.shape[1], bool), sample=-1, sol=-1, models=0)
    hom = lambda x: np.vstack([x, np.ones((1, x.shape[1]))])
    for si, smp in enumerate(np.asarray(samples)):
        try:
            Es = essmat5(hom(x1[:, smp]), hom(x2[:, smp]))
        except np.linalg.LinAlgError:
            continue
        for k in range(Es.shape[1]):
            if not np.all(np.isfinite(Es[:, k])):
                continue
            best['models'] += 1
            m = sampson2(Es[:, k], x1, x2) < thr2
            if m.sum() > best['count']:
                best.update(e=Es[:, k].copy(), count=int(m.sum()), mask=m, sample=si, sol=k)
    return best


# ---- the synthetic pair of the tests ---------------------------------------------------------------------------------

def rodrigues(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def synthetic_pair(rng, n, front=1, noise=0.0, t_scale=1.0):
    """Points uniform in a 4 x 4 x 2 box at distance 6 along front * z, rotation vector 0.15 N(0, I), unit baseline in a
    random direction (times t_scale): dict(x1, x2 (2 x n, normalised), R, t, X (camera-1 frame), e (unit, the layout
    above), E = [t]x R)."""
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), front * rng.uniform(5, 7, n)])
    R = rodrigues(0.15 * rng.normal(size=3))
    t = rng.normal(size=3)
    t = t_scale * t / np.linalg.norm(t)
    Y = R @ X + t[:, None]
    x1, x2 = X[:2] / X[2], Y[:2] / Y[2]
    if noise:
        x1 = x1 + noise * rng.normal(size=x1.shape)
        x2 = x2 + noise * rng.normal(size=x2.shape)
    Tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = Tx @ R                                                   # x2' E x1 = 0
    e = E.reshape(-1)                                            # e[a + 3 b] = E[b, a]: row-major E
    nrm = np.linalg.norm(e)
    return dict(x1=x1, x2=x2, R=R, t=t, X=X, E=E, e=e / nrm if nrm > 0 else e)


def dist_to(e_true, Es):
    """Distance of the nearest column of Es (9 x k) to the unit vector e_true, up to sign; inf without a column."""
    if Es.shape[1] == 0:
        return np.inf
    return float(np.min(np.minimum(np.linalg.norm(Es - e_true[:, None], axis=0), np.linalg.norm(Es + e_true[:, None], axis=0))))


def residuals(e, Q1, Q2):
    """(max |q2' E q1| over the set, |det E|, max |2 E E' E - tr(E E') E|) of a unit solution."""
    M = np.asarray(e).reshape(3, 3).T
    epi = np.max(np.abs(np.sum(Q1 * (M @ Q2), 0)))
    return float(epi), float(abs(np.linalg.det(M))), float(np.max(np.abs(2 * M @ M.T @ M - np.trace(M @ M.T) * M)))
