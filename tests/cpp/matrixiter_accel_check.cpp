// matrixiter_accel_check.cpp -- include/mmadmm/MatrixIter.h with the ORTHOMIN and CG accelerators
// (ParamIter.iaccel = 1 / -1) and row scaling (iscal = 1) on a 226-row banded system, through
// SparseItObj::MatrixIter as a caller of the reference's lib/LASolver would write it.  Test
// infrastructure (tests/test_cpp_matrixiter_accel.py; needs a GPU).  Prints one
// "name ok|FAIL detail" line per check.
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "SparseItObj.h"

using namespace SparseItObj;

static int fails = 0;
static void check(const char* name, bool ok, const std::string& why = "") {
    std::printf("%s %s %s\n", name, ok ? "ok" : "FAIL", why.c_str());
    if (!ok) fails++;
}

// ||b - A x|| / ||b|| from the host arrays
static double residual(MatrixIter& m, const std::vector<double>& b, std::vector<double>& x) {
    double r2 = 0.0, b2 = 0.0;
    for (int i = 0; i < m.get_n(); ++i) {
        const double r = b[i] - m.mult_row(i, x.data());
        r2 += r * r;
        b2 += b[i] * b[i];
    }
    return std::sqrt(r2 / b2);
}

int main() {
    const int n = 226, band = 15;
    MatrixStruc s(n, 0);
    for (int i = 0; i < n; ++i)
        for (int j : {i - band, i - 1, i + 1, i + band})
            if (j >= 0 && j < n) s.set_entry(i, j);
    s.pack();
    try {
        MatrixIter m(s);
        std::vector<double> b(n), x(n);
        // sym: off-diagonals a_ij = a_ji; otherwise the lower ones differ from the upper ones
        auto fill = [&](bool sym) {
            m.zeroa();
            for (int i = 0; i < n; ++i) {
                double sum = 0.0;
                for (int k = m.rowBegin(i); k < m.rowEndPlusOne(i); ++k) {
                    const int j = m.getColIndex(k);
                    if (j == i) continue;
                    const int lo = i < j ? i : j;
                    double v = -1.0 - 0.25 * std::sin(1.0 + lo) * ((j - i == 1 || i - j == 1) ? 1.0 : 0.5);
                    if (!sym && j < i) v *= 0.6;
                    m.aValue(k) = v;
                    sum += std::fabs(v);
                }
                m.aValue(i, i) = sum + 0.5;
                b[i] = std::cos(0.37 * i) + 0.1;
                m.bValue(i) = b[i];
            }
        };
        ParamIter p;
        p.order = 0;
        p.level = 0;
        p.iscal = 0;
        p.nitmax = 500;
        p.resid_reduc = 1.e-8;
        m.sfac(p);
        int nitr = 0;

        fill(false);
        p.iaccel = 1;
        p.north = 5;
        m.solve(p, x.data(), nitr);
        double r = residual(m, b, x);
        check("orthomin", nitr > 0 && r < p.resid_reduc, "nitr " + std::to_string(nitr) + " residual " + std::to_string(r * 1e8) + "e-8");

        p.iscal = 1;  // rows scaled by their diagonal on the device; the host arrays stay unscaled
        m.solve(p, x.data(), nitr);
        r = residual(m, b, x);
        const std::vector<double> f = m.get_scale();
        bool fok = true;
        for (int i = 0; i < n; ++i) fok = fok && f[i] == 1.0 / (m.aValue(i, i) + 1.0e-300);
        check("orthomin_scaled", nitr > 0 && r < 10 * p.resid_reduc && fok && p.iscal == 1,
              "nitr " + std::to_string(nitr) + " residual " + std::to_string(r * 1e8) + "e-8");

        fill(true);
        p.iaccel = -1;  // conjugate gradients: the solve resets iscal, as the reference does
        m.solve(p, x.data(), nitr);
        r = residual(m, b, x);
        check("cg", nitr > 0 && r < p.resid_reduc, "nitr " + std::to_string(nitr) + " residual " + std::to_string(r * 1e8) + "e-8");
        check("cg_resets_iscal", p.iscal == 0);

        p.iaccel = 1;
        p.north = 0;
        bool threw = false;
        try {
            m.solve(p, x.data(), nitr);
        } catch (const General_Exception& e) {
            threw = std::string(e.p).find("north") != std::string::npos;
        }
        check("north_0_throws", threw);
    } catch (const General_Exception& e) {
        check("no_exception", false, e.p);
    }
    return fails ? 1 : 0;
}
