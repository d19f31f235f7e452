"""Robust pose-graph optimisation of a sequence of fragments (Choi, Zhou, Koltun 2015: line processes over the loop
closures), and the writers of the `gt.log` / `gt.info` pair `evaluate.read_log` / `read_info_file` parse.

Host code, NumPy float64, dense: the graph of a sequence has a few hundred nodes at most, 6 (N - 1) unknowns, and one
solve takes milliseconds next to the seconds of a pairwise registration.  It is not a hot path and stays off the GPU.

This is the project's own statement of the cost.  Open3D's `GlobalOptimization` is not available here and has not been
compared; what is recalled from it is marked [RECALLED].

Conventions (those of `gt.log`):
  node pose X_i maps fragment i into the world; node 0 is fixed at the identity;
  edge (i, j, T_ij, L_ij, uncertain): T_ij maps points of fragment j into fragment i's frame;
  L_ij = matching.information_matrix(src = fragment j, dst = fragment i, T = T_ij), rotation first.

The cost.  D = X_i^-1 X_j T_ij^-1 (the identity when the edge is satisfied; it acts in fragment i's frame, where L_ij's
points live), e = (alpha, beta, gamma, t) with D.R = Rz(gamma) Ry(beta) Rx(alpha): alpha = atan2(R21, R22), beta =
-asin(clip R20), gamma = atan2(R10, R00), the parametrisation of ICP's update; f = e^T L e;
  E = sum_certain f + sum_uncertain [ l f + mu (sqrt l - 1)^2 ],
with l = (mu / (mu + f))^2 in closed form before every linearisation, and
  mu = preference_loop_closure * max_corr_dist^2 * mean over the uncertain edges of L[5, 5] (their correspondence count)
[RECALLED: Open3D's line-process weight].

The solver.  Levenberg-Marquardt on right-multiplied updates X_n <- X_n U(d_n), U = [Rz(d2) Ry(d1) Rx(d0) | d3 d4 d5], n >=
1; the Jacobians are central differences (step 1e-6) of e; with l held at its closed form the normal equations are those of
the weighted least-squares problem.  A step is accepted only when E (with l re-closed) does not rise, otherwise the damping
grows tenfold; it stops on a relative decrease of E <= 1e-12 or after max_iteration linearisations.  After convergence the
uncertain edges with l < edge_prune_threshold are dropped and the rest is optimised again.
"""
from collections import deque, namedtuple

import numpy as np

Edge = namedtuple("Edge", ["i", "j", "T", "info", "uncertain", "fitness"])
_STEP = 1e-6


def euler_matrix(d):
    """[..., 4, 4] U = [Rz(d2) Ry(d1) Rx(d0) | d3 d4 d5] of d [..., 6]."""
    d = np.asarray(d, np.float64)
    ca, sa, cb, sb, cg, sg = np.cos(d[..., 0]), np.sin(d[..., 0]), np.cos(d[..., 1]), np.sin(d[..., 1]), np.cos(d[..., 2]), \
        np.sin(d[..., 2])
    U = np.zeros(d.shape[:-1] + (4, 4))
    U[..., 0, 0] = cg * cb; U[..., 0, 1] = cg * sb * sa - sg * ca; U[..., 0, 2] = cg * sb * ca + sg * sa
    U[..., 1, 0] = sg * cb; U[..., 1, 1] = sg * sb * sa + cg * ca; U[..., 1, 2] = sg * sb * ca - cg * sa
    U[..., 2, 0] = -sb;     U[..., 2, 1] = cb * sa;                U[..., 2, 2] = cb * ca
    U[..., :3, 3] = d[..., 3:]
    U[..., 3, 3] = 1.0
    return U


def euler_vector(D):
    """e [..., 6] = (alpha, beta, gamma, t) of D [..., 4, 4], the inverse of euler_matrix."""
    D = np.asarray(D, np.float64)
    e = np.empty(D.shape[:-2] + (6,))
    e[..., 0] = np.arctan2(D[..., 2, 1], D[..., 2, 2])
    e[..., 1] = -np.arcsin(np.clip(D[..., 2, 0], -1.0, 1.0))
    e[..., 2] = np.arctan2(D[..., 1, 0], D[..., 0, 0])
    e[..., 3:] = D[..., :3, 3]
    return e


def rigid_inverse(T):
    """[..., 4, 4] inverse of rigid matrices [R | t]: [R^T | -R^T t]."""
    T = np.asarray(T, np.float64)
    out = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -np.einsum("...ab,...b->...a", Rt, T[..., :3, 3])
    out[..., 3, 3] = 1.0
    return out


class PoseGraph:
    """n_nodes fragments and the registered pairs between them."""

    def __init__(self, n_nodes):
        if int(n_nodes) < 1:
            raise ValueError(f"n_nodes must be >= 1, got {n_nodes}")
        self.n_nodes = int(n_nodes)
        self.edges = []

    def add_edge(self, i, j, T, info, uncertain, fitness=1.0):
        """T [4, 4] maps fragment j's points into fragment i's frame; info [6, 6], rotation first."""
        i, j = int(i), int(j)
        if not (0 <= i < self.n_nodes and 0 <= j < self.n_nodes) or i == j:
            raise ValueError(f"edge ({i}, {j}) in a graph of {self.n_nodes} nodes")
        T = np.array(T, np.float64).reshape(4, 4)
        info = np.array(info, np.float64).reshape(6, 6)
        if not (np.isfinite(T).all() and np.isfinite(info).all()):
            raise ValueError(f"edge ({i}, {j}): T and info must be finite")
        self.edges.append(Edge(i, j, T, info, bool(uncertain), float(fitness)))

    def traversal_order(self):
        """Edge numbers in the order the initial poses take them: certain first, then higher fitness, then (i, j)."""
        return sorted(range(len(self.edges)), key=lambda k: (self.edges[k].uncertain, -self.edges[k].fitness,
                                                             self.edges[k].i, self.edges[k].j))

    def initial_poses(self):
        """[N, 4, 4]: breadth-first from node 0 over the edges in traversal_order, X_j = X_i T_ij (X_i = X_j T_ij^-1
        against the edge's direction).  A node that cannot be reached is NaN."""
        X = np.full((self.n_nodes, 4, 4), np.nan)
        X[0] = np.eye(4)
        order = self.traversal_order()
        queue, seen = deque([0]), {0}
        while queue:
            a = queue.popleft()
            for k in order:
                ed = self.edges[k]
                if ed.i == a and ed.j not in seen:
                    X[ed.j] = X[a] @ ed.T
                    seen.add(ed.j)
                    queue.append(ed.j)
                elif ed.j == a and ed.i not in seen:
                    X[ed.i] = X[a] @ rigid_inverse(ed.T)
                    seen.add(ed.i)
                    queue.append(ed.i)
        return X


def _residuals(X, ei, ej, Tinv):
    """D [E, 4, 4] and e [E, 6] of every edge."""
    D = rigid_inverse(X[ei]) @ X[ej] @ Tinv
    return D, euler_vector(D)


def _line_process(f, unc, mu):
    """(l per edge, E): l = (mu / (mu + f))^2 on the uncertain edges, 1 on the others."""
    l = np.ones_like(f)
    if unc.any():
        l[unc] = (mu / (mu + f[unc])) ** 2
    E = f[~unc].sum() + (l[unc] * f[unc] + mu * (np.sqrt(l[unc]) - 1.0) ** 2).sum()
    return l, float(E)


def _optimize_once(X, ei, ej, Tinv, info, unc, mu, free, max_iteration):
    """Levenberg-Marquardt over the nodes `free` (node numbers); returns (X, l, the E of the start and of every accepted
    step)."""
    col = -np.ones(len(X), np.int64)
    col[free] = np.arange(len(free))
    n_unk = 6 * len(free)
    basis = np.concatenate([np.eye(6) * _STEP, -np.eye(6) * _STEP])          # [12, 6]
    U = euler_matrix(basis)                                                  # [12, 4, 4]
    Uinv = rigid_inverse(U)

    def cost(Xc):
        _, e = _residuals(Xc, ei, ej, Tinv)
        f = np.einsum("ka,kab,kb->k", e, info, e)
        l, E = _line_process(f, unc, mu)
        return e, l, E

    e, l, E = cost(X)
    history = [E]
    if n_unk == 0 or len(ei) == 0:
        return X, l, history
    lam = 1e-4
    for _ in range(int(max_iteration)):
        # X_i <- X_i U: D' = U^-1 D;  X_j <- X_j U: D' = (X_i^-1 X_j) U T_ij^-1
        A = rigid_inverse(X[ei]) @ X[ej]
        D = A @ Tinv
        ei_pert = euler_vector(Uinv[None, :, :, :] @ D[:, None, :, :])                       # [E, 12, 6]
        ej_pert = euler_vector(A[:, None, :, :] @ U[None, :, :, :] @ Tinv[:, None, :, :])
        Ji = np.swapaxes(ei_pert[:, :6] - ei_pert[:, 6:], 1, 2) / (2.0 * _STEP)              # [E, 6 (e), 6 (delta)]
        Jj = np.swapaxes(ej_pert[:, :6] - ej_pert[:, 6:], 1, 2) / (2.0 * _STEP)
        H = np.zeros((n_unk, n_unk))
        g = np.zeros(n_unk)
        W = l[:, None, None] * info
        for k in range(len(ei)):
            blocks = [(col[ei[k]], Ji[k]), (col[ej[k]], Jj[k])]
            We = W[k] @ e[k]
            for ca, Ja in blocks:
                if ca < 0:
                    continue
                g[6 * ca:6 * ca + 6] += Ja.T @ We
                for cb, Jb in blocks:
                    if cb >= 0:
                        H[6 * ca:6 * ca + 6, 6 * cb:6 * cb + 6] += Ja.T @ W[k] @ Jb
        diag = np.diag(H).copy()
        diag[diag <= 0.0] = 1.0
        accepted = False
        while lam < 1e16:
            try:
                step = np.linalg.solve(H + lam * np.diag(diag), -g)
            except np.linalg.LinAlgError:
                lam *= 10.0
                continue
            Xn = X.copy()
            Xn[free] = X[free] @ euler_matrix(step.reshape(-1, 6))
            en, ln, En = cost(Xn)
            if np.isfinite(En) and En <= E:
                accepted = True
                break
            lam *= 10.0
        if not accepted:
            break
        decrease = E - En
        X, e, l = Xn, en, ln
        history.append(En)
        lam = max(lam * 0.1, 1e-15)
        done = decrease <= 1e-12 * E
        E = En
        if done:
            break
    return X, l, history


def optimize(graph, max_corr_dist, preference_loop_closure=1.0, edge_prune_threshold=0.25, max_iteration=100, init=None):
    """Optimise the node poses of `graph`.  init: [N, 4, 4] starting poses (NaN = unreached), default
    graph.initial_poses().  Returns (poses [N, 4, 4] with X_0 the identity and NaN for the nodes no edge path reaches from
    node 0, l per edge -- 1 on certain edges, the value that decided on pruned ones, NaN on edges of an unreached node --,
    kept bool per edge, the list of E at the start and after every accepted step of both passes)."""
    X = np.array(graph.initial_poses() if init is None else init, np.float64).reshape(graph.n_nodes, 4, 4)
    X[0] = np.eye(4)
    n_edges = len(graph.edges)
    reached = np.isfinite(X).all((1, 2))
    ei = np.array([ed.i for ed in graph.edges], np.int64)
    ej = np.array([ed.j for ed in graph.edges], np.int64)
    unc = np.array([ed.uncertain for ed in graph.edges], bool)
    l_out = np.full(n_edges, np.nan)
    kept = np.zeros(n_edges, bool)
    if n_edges == 0:
        return X, l_out, kept, []
    live = reached[ei] & reached[ej]
    Tinv = rigid_inverse(np.stack([ed.T for ed in graph.edges]))
    info = np.stack([ed.info for ed in graph.edges])
    mu = 0.0
    if (unc & live).any():
        mu = float(preference_loop_closure) * float(max_corr_dist) ** 2 * float(info[unc & live][:, 5, 5].mean())
    free = np.flatnonzero(reached)[1:]                                       # node 0 is reached and fixed
    history = []
    use = np.flatnonzero(live)
    X, l, h = _optimize_once(X, ei[use], ej[use], Tinv[use], info[use], unc[use], mu, free, max_iteration)
    history += h
    l_out[use] = l
    kept[use] = ~unc[use] | (l >= edge_prune_threshold)
    if (~kept[use]).any():
        use2 = np.flatnonzero(kept)
        X, l, h = _optimize_once(X, ei[use2], ej[use2], Tinv[use2], info[use2], unc[use2], mu, free, max_iteration)
        history += h
        l_out[use2] = l
    X[0] = np.eye(4)
    return X, l_out, kept, history


def benchmark_order(info):
    """A rotation-first matrix in the block order of the 3DMatch benchmark's gt.info (translation first, the order
    evaluate.compute_transform_error reads), and back: the permutation is its own inverse."""
    p = [3, 4, 5, 0, 1, 2]
    return np.asarray(info)[np.ix_(p, p)]


def _write_blocks(path, records, rows):
    with open(path, "w") as fh:
        for i, j, n, M in records:
            M = np.asarray(M, np.float64).reshape(rows, -1)
            fh.write(f"{int(i)}\t{int(j)}\t{int(n)}\n")
            for row in M:
                fh.write("\t".join("%.17g" % v for v in row) + "\n")


def write_log(path, records):
    """records: (i, j, n, T [4, 4]) -> the `gt.log` format evaluate.read_log parses."""
    _write_blocks(path, records, 4)


def write_info(path, records):
    """records: (i, j, n, info [6, 6]) -> the `gt.info` format evaluate.read_info_file parses (as float32)."""
    _write_blocks(path, records, 6)
