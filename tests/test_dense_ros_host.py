"""Host check of csrc/dense_ros.hpp, the stage program of the dense Ros1..Ros4 drivers, compiled with g++ into a stand-alone program (no GPU,
no HIP) behind a small host back end: column-major std::vector matrices, naive gemm / comb / copy, factor keeps F, and solve forms
(E' (x) F' + F' (x) E') vec X = -vec R, solves it by Gaussian elimination with partial pivoting and symmetrises.

The program's X(t_i) and K(t_i) are compared with the oracle's solve_dense_ros1..4 on _adaptive_ros2_model.stiff_pencil(n, seed), n in {4, 6},
seed in {1, 3}, tspan (1, 0), dt = -0.25 (four steps), from X0 = 0 and from one symmetric positive definite X0.  Bound: delta < 1e-10 on every
X(t_i) and K(t_i) (delta relative to the larger norm, as D.delta), the bound of test_ros3_ros4_against_oracle.  Replacing the oracle's Lyapunov
solver by this Kronecker solve moves the four trajectories by a few 1e-15 on these pencils (cond(E) <= 3).

The adaptive driver's use of the program, the order-2 ros_stages without ros_combine followed by k_step_error's X + a2 K2 + a1 K1, is run as
the program's "split" mode and must reproduce the full step bit for bit: both modes do the same floating-point operations in the same order
(the program is compiled with -ffp-contract=off, so that no compiler fuses one of the two sums and not the other)."""
import os
import subprocess

import numpy as np
import pytest

import dre_amd as D
import dre_oracle as o
from _adaptive_ros2_model import stiff_pencil
from conftest import ROOT

CSRC = os.path.join(ROOT, "differentialriccatiequations.jl_amd", "csrc")

SRC = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dense_ros.hpp"

struct HM {                                   // column-major, ld = r
    int r = 0, c = 0;
    std::vector<double> a;
    void shape(int rows, int cols) { r = rows; c = cols; a.assign((size_t)rows * cols, 0.0); }
    double& at(int i, int j) { return a[(size_t)i + (size_t)j * r]; }
    double at(int i, int j) const { return a[(size_t)i + (size_t)j * r]; }
};

struct HostOps {
    using M = HM;
    const HM* E = nullptr;
    HM F;
    int solves = 0;
    void gemm(bool tA, bool tB, double alpha, const HM& A, const HM& B, double beta, HM& C) {
        const int m = tA ? A.c : A.r, k = tA ? A.r : A.c, n = tB ? B.r : B.c, k2 = tB ? B.c : B.r;
        if (k != k2) { std::printf("gemm: inner dimensions %d, %d\n", k, k2); std::exit(2); }
        if (beta == 0.0) C.shape(m, n);
        if (C.r != m || C.c != n) { std::printf("gemm: C is %d x %d, expected %d x %d\n", C.r, C.c, m, n); std::exit(2); }
        HM out = C;
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < m; ++i) {
                double s = 0.0;
                for (int l = 0; l < k; ++l) s += (tA ? A.at(l, i) : A.at(i, l)) * (tB ? B.at(j, l) : B.at(l, j));
                out.at(i, j) = alpha * s + (beta == 0.0 ? 0.0 : beta * C.at(i, j));
            }
        C = out;
    }
    void comb(HM& out, double a0, const HM& M0, double a1, const HM* M1, double a2, const HM* M2, bool sym) {
        HM v; v.shape(M0.r, M0.c);
        for (size_t i = 0; i < v.a.size(); ++i) v.a[i] = a0 * M0.a[i] + (M1 ? a1 * M1->a[i] : 0.0) + (M2 ? a2 * M2->a[i] : 0.0);
        if (sym) {
            HM s = v;
            for (int j = 0; j < v.c; ++j) for (int i = 0; i < v.r; ++i) s.at(i, j) = 0.5 * (v.at(i, j) + v.at(j, i));
            v = s;
        }
        out = v;
    }
    void copy(const HM& src, HM& dst) { dst = src; }
    void factor(const HM& Fm) { F = Fm; }
    // (E' (x) F' + F' (x) E') vec X = -vec R
    void solve(const HM& R, HM& X) {
        ++solves;
        const int n = R.r, N = n * n;
        std::vector<double> K((size_t)N * N), b((size_t)N);
        for (int j = 0; j < n; ++j) for (int i = 0; i < n; ++i) {
            b[(size_t)i + (size_t)n * j] = -R.at(i, j);
            for (int l = 0; l < n; ++l) for (int k = 0; k < n; ++k)
                K[((size_t)i + (size_t)n * j) * N + ((size_t)k + (size_t)n * l)] = E->at(l, j) * F.at(k, i) + F.at(l, j) * E->at(k, i);
        }
        for (int c = 0; c < N; ++c) {                      // row-major K: elimination with partial pivoting
            int pv = c;
            for (int r = c + 1; r < N; ++r) if (std::abs(K[(size_t)r * N + c]) > std::abs(K[(size_t)pv * N + c])) pv = r;
            if (K[(size_t)pv * N + c] == 0.0) { std::printf("solve: singular\n"); std::exit(2); }
            if (pv != c) { for (int j = 0; j < N; ++j) std::swap(K[(size_t)pv * N + j], K[(size_t)c * N + j]); std::swap(b[pv], b[c]); }
            for (int r = c + 1; r < N; ++r) {
                const double f = K[(size_t)r * N + c] / K[(size_t)c * N + c];
                if (f == 0.0) continue;
                for (int j = c; j < N; ++j) K[(size_t)r * N + j] -= f * K[(size_t)c * N + j];
                b[r] -= f * b[c];
            }
        }
        for (int r = N - 1; r >= 0; --r) {
            double s = b[r];
            for (int j = r + 1; j < N; ++j) s -= K[(size_t)r * N + j] * b[j];
            b[r] = s / K[(size_t)r * N + r];
        }
        HM v; v.shape(n, n);
        for (int j = 0; j < n; ++j) for (int i = 0; i < n; ++i) v.at(i, j) = 0.5 * (b[(size_t)i + (size_t)n * j] + b[(size_t)j + (size_t)n * i]);
        X = v;
    }
};

static HM read_mat(FILE* f, int r, int c) {
    HM m; m.shape(r, c);
    for (double& v : m.a) if (std::fscanf(f, "%lf", &v) != 1) { std::printf("short input\n"); std::exit(2); }
    return m;
}
static void print_mat(const char* what, int i, const HM& m) {
    std::printf("%s %d", what, i);
    for (double v : m.a) std::printf(" %.17g", v);
    std::printf("\n");
}

// usage: prog INPUT full|split
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    const bool split = std::strcmp(argv[2], "split") == 0;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int n, m, q, order, nsteps;
    double t0, dt;
    if (std::fscanf(f, "%d %d %d %d %d %lf %lf", &n, &m, &q, &order, &nsteps, &t0, &dt) != 7) return 2;
    const HM E = read_mat(f, n, n), A = read_mat(f, n, n), B = read_mat(f, n, m), C = read_mat(f, q, n);
    HM X = read_mat(f, n, n), CtC, Kt;
    std::fclose(f);
    HostOps ops;
    ops.E = &E;
    dre::RosWork<HM> w;
    ops.gemm(true, false, 1.0, C, C, 0.0, CtC);
    const dre::RosOperands<HM> p{E, A, B, CtC};
    dre::ros_EtKB(ops, p, w, X, Kt);
    print_mat("X", 0, X);
    print_mat("K", 0, Kt);
    for (int i = 1; i <= nsteps; ++i) {
        const double tau = (t0 + (i - 1) * dt) - (t0 + i * dt);
        dre::ros_stages(ops, order, tau, p, X, Kt, w);
        if (split) {                                       // the adaptive driver's own combination (k_step_error)
            if (order != 2) return 2;
            const double a2 = dre::ros2_weight_k2(tau), a1 = dre::ros2_weight_k1(tau);
            for (size_t e = 0; e < X.a.size(); ++e) X.a[e] = X.a[e] + a2 * w.K2.a[e] + a1 * w.K1.a[e];
        } else {
            dre::ros_combine(ops, order, tau, X, w);
        }
        dre::ros_EtKB(ops, p, w, X, Kt);
        print_mat("X", i, X);
        print_mat("K", i, Kt);
    }
    std::printf("solves %d\n", ops.solves);
    return 0;
}
"""

NSTEPS, T0, DT = 4, 1.0, -0.25


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("dense_ros")
    cpp = d / "dense_ros_host.cpp"
    cpp.write_text(SRC)
    exe = d / "dense_ros_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", CSRC, str(cpp), "-o", str(exe)], check=True)
    return d, exe


def _x0(n, seed, spd):
    if not spd:
        return np.zeros((n, n))
    G = np.random.default_rng(100 + seed).standard_normal((n, n))
    return G @ G.T / n + 0.5 * np.eye(n)


def _run(program, E, A, B, C, X0, order, mode):
    d, exe = program
    n, m, q = E.shape[0], B.shape[1], C.shape[0]
    inp = d / "case.txt"
    with open(inp, "w") as f:
        f.write(f"{n} {m} {q} {order} {NSTEPS} {T0!r} {DT!r}\n")
        for M in (E, A, B, C, X0):
            f.write(" ".join(repr(float(v)) for v in np.asarray(M).flatten(order="F")) + "\n")
    r = subprocess.run([str(exe), str(inp), mode], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    Xs, Ks, solves = [], [], None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "solves":
            solves = int(w[1])
            continue
        v = np.array([float(x) for x in w[2:]])
        if w[0] == "X":
            Xs.append(v.reshape((n, n), order="F"))
        else:
            Ks.append(v.reshape((n, m), order="F").T)           # the program holds K(t)' (n x m)
    assert len(Xs) == len(Ks) == NSTEPS + 1
    return Xs, Ks, solves


@pytest.mark.parametrize("spd", [False, True], ids=["X0=0", "X0=spd"])
@pytest.mark.parametrize("order", [1, 2, 3, 4])
@pytest.mark.parametrize("n,seed", [(4, 1), (4, 3), (6, 1), (6, 3)])
def test_stage_program_against_the_oracle(program, n, seed, order, spd):
    E, A, B, C = stiff_pencil(n, seed=seed)
    X0 = _x0(n, seed, spd)
    Xs, Ks, solves = _run(program, E, A, B, C, X0, order, "full")
    assert solves == NSTEPS * order                              # one stage solve per order and step, all on one factorisation
    oracle = (o.solve_dense_ros1, o.solve_dense_ros2, o.solve_dense_ros3, o.solve_dense_ros4)[order - 1]
    ref = oracle(o.GDREProblem(E, A, B, C, X0, (T0, T0 + NSTEPS * DT)), dt=DT, save_state=True)
    assert len(ref.X) == len(ref.K) == NSTEPS + 1
    worst = 0.0
    for i in range(NSTEPS + 1):
        dX = 0.0 if i == 0 and not spd else D.delta(Xs[i], ref.X[i])      # (X0 = 0: both are exactly zero, delta is 0 / 0)
        dK = 0.0 if i == 0 and not spd else D.delta(Ks[i], ref.K[i])
        worst = max(worst, dX, dK)
        assert dX < 1e-10 and dK < 1e-10, (i, dX, dK)
    print(f"n = {n}, seed = {seed}, order {order}, spd = {spd}: largest delta {worst:.2e}")
    if not spd:
        assert not Xs[0].any() and not Ks[0].any() and not np.asarray(ref.X[0]).any() and not np.asarray(ref.K[0]).any()


@pytest.mark.parametrize("spd", [False, True], ids=["X0=0", "X0=spd"])
@pytest.mark.parametrize("n,seed", [(4, 1), (4, 3), (6, 1), (6, 3)])
def test_order_2_stages_with_the_callers_combination_are_the_full_step(program, n, seed, spd):
    E, A, B, C = stiff_pencil(n, seed=seed)
    X0 = _x0(n, seed, spd)
    Xf, Kf, _ = _run(program, E, A, B, C, X0, 2, "full")
    Xs, Ks, solves = _run(program, E, A, B, C, X0, 2, "split")
    assert solves == 2 * NSTEPS
    for i in range(1, NSTEPS + 1):
        assert np.array_equal(Xs[i], Xf[i]) and np.array_equal(Ks[i], Kf[i]), (i, D.delta(Xs[i], Xf[i]), D.delta(Ks[i], Kf[i]))
