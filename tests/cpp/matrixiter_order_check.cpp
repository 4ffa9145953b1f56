// matrixiter_order_check.cpp -- include/mmadmm/MatrixIter.h with an ordered ILU: rcm() and
// MatrixIter::set_user_ordering_vector under the reference's names, on a 226-row banded system,
// through SparseItObj::MatrixIter as a caller of the reference's lib/LASolver would write it.  Test
// infrastructure (tests/test_cpp_matrixiter_order.py; needs a GPU).  Prints one
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
        std::vector<double> b(n), x(n), xnat(n);
        for (int i = 0; i < n; ++i) {
            double sum = 0.0;
            for (int k = m.rowBegin(i); k < m.rowEndPlusOne(i); ++k) {
                const int j = m.getColIndex(k);
                if (j == i) continue;
                const int lo = i < j ? i : j;
                double v = -1.0 - 0.25 * std::sin(1.0 + lo) * ((j - i == 1 || i - j == 1) ? 1.0 : 0.5);
                if (j < i) v *= 0.6;
                m.aValue(k) = v;
                sum += std::fabs(v);
            }
            m.aValue(i, i) = sum + 0.5;
            b[i] = std::cos(0.37 * i) + 0.1;
            m.bValue(i) = b[i];
        }

        // the free rcm() of the reference: a permutation of 0 .. n - 1
        std::vector<int> lorder(n, -1), seen(n, 0);
        rcm(m.get_ia(), m.get_ja(), n, lorder.data());
        bool perm = true;
        for (int i = 0; i < n; ++i) {
            perm = perm && lorder[i] >= 0 && lorder[i] < n && !seen[lorder[i]];
            if (perm) seen[lorder[i]] = 1;
        }
        check("rcm_is_a_permutation", perm);

        // ParamIter as constructed (order 1) is refused while no ordering is set ...
        ParamIter p;
        p.level = 0;
        p.iscal = 0;
        p.nitmax = 500;
        p.resid_reduc = 1.e-8;
        bool threw = false;
        try {
            m.sfac(p);
        } catch (const General_Exception& e) {
            threw = std::string(e.p).find("unsupported ParamIter.order") != std::string::npos;
        }
        check("order_1_alone_throws", threw);

        // ... and is what the reference's defaults mean once the RCM vector is set
        int nitr = 0;
        m.set_user_ordering_vector(nullptr);  // a null pointer changes nothing
        m.set_user_ordering_vector(lorder.data());
        m.sfac(p);
        m.solve(p, x.data(), nitr);
        double r = residual(m, b, x);
        check("cgstab_rcm", p.order == 1 && nitr > 0 && r < p.resid_reduc,
              "nitr " + std::to_string(nitr) + " residual " + std::to_string(r * 1e8) + "e-8");

        p.iaccel = 1;
        p.north = 5;
        m.solve(p, x.data(), nitr);
        r = residual(m, b, x);
        check("orthomin_rcm", nitr > 0 && r < p.resid_reduc,
              "nitr " + std::to_string(nitr) + " residual " + std::to_string(r * 1e8) + "e-8");

        // a repeated index is the reference's error_4, an index out of range its error_3
        std::vector<int> bad(lorder);
        bad[3] = bad[7];
        threw = false;
        try {
            m.set_user_ordering_vector(bad.data());
        } catch (const General_Exception& e) {
            threw = std::string(e.p).find("error_4 in user ordering") != std::string::npos;
        }
        check("repeated_index_throws", threw);
        bad = lorder;
        bad[n - 1] = n;
        threw = false;
        try {
            m.set_user_ordering_vector(bad.data());
        } catch (const General_Exception& e) {
            threw = std::string(e.p).find("error_3 in user ordering") != std::string::npos;
        }
        check("out_of_range_throws", threw);
        // the refused vectors left the ordering in place
        m.sfac(p);
        m.solve(p, xnat.data(), nitr);
        bool same = true;
        for (int i = 0; i < n; ++i) same = same && xnat[i] == x[i];
        check("refused_vector_keeps_ordering", same && nitr > 0);
    } catch (const General_Exception& e) {
        check("no_exception", false, e.p);
    }
    return fails ? 1 : 0;
}
