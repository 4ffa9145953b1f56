// fields_check.cpp -- MeshIntegrator<D>::regridFromFields / regridFromFieldsHuang (include/mmadmm/
// MeshIntegrator.h) with a host array and with a device array, alpha solved and given, against the
// host-only mmadmm_fields_monitor followed by regridFromValues on a second engine: the alphas and the
// rebuilt monitor grids must be equal bit for bit.  Prints one "<name> ok|FAIL" line per check.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "MeshIntegrator.h"
#include "MeshUtils.h"

template <int D>
class Identity : public MonitorFunction<D> {
public:
    void operator()(Eigen::Vector<double, D> &x, Eigen::Matrix<double, D, D> &M) override {
        (void)x;
        M.setZero();
        for (int i = 0; i < D; i++) M(i, i) = 1.0;
    }
};

static int fails = 0;
static void report(const std::string &name, bool ok) {
    printf("%s %s\n", name.c_str(), ok ? "ok" : "FAIL");
    if (!ok) fails++;
}

static std::vector<double> grid_of(mmadmm_handle h) {
    int nP = 0, nF = 0, rows = 0;
    mmadmm_cxx::check(mmadmm_sizes(h, &nP, &nF, &rows));
    std::vector<double> g((size_t)rows * 9, -1.0);  // rows x D*D used; the tail keeps its fill in 2D
    mmadmm_cxx::check(mmadmm_get(h, "grid", g.data()));
    return g;
}
static bool same(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * 8) == 0;
}

template <int D>
static void run(int n) {
    std::unordered_map<std::string, double> p{{"nx", (double)n}, {"ny", (double)n}, {"nz", (double)n}, {"xa", 0},
                                              {"xb", 1},         {"ya", 0},         {"yb", 1},         {"za", 0},
                                              {"zb", 1}};
    Eigen::MatrixXd V;
    Eigen::MatrixXi F;
    std::vector<NodeType> mask;
    utils::generateUniformRectMesh<D>(p, &V, &F, &mask, NodeType::BOUNDARY_FIXED);
    Identity<D> mon;
    Mesh<D> meshA(V, F, mask, &mon, 1, 1000.0, 0.0, 0.5, 0, false);
    Mesh<D> meshB(V, F, mask, &mon, 1, 1000.0, 0.0, 0.5, 0, false);
    MeshIntegrator<D> A(0.025, meshA), B(0.025, meshB);
    int nP = 0, nF = 0, rows = 0;
    mmadmm_cxx::check(mmadmm_sizes(A.handle(), &nP, &nF, &rows));

    // the engine's own positions and simplices: what the host function must be given
    constexpr int C = D + 1;  // one full batch of the first recovery and a remainder of one
    std::vector<double> X((size_t)nP * D), U((size_t)nP * C), M((size_t)nP * D * D);
    std::vector<int32_t> f((size_t)nF * (D + 1));
    mmadmm_cxx::check(mmadmm_get(A.handle(), "points", X.data()));
    mmadmm_cxx::check(mmadmm_get_simplices(A.handle(), f.data()));
    for (int v = 0; v < nP; v++) {
        const double *x = &X[(size_t)v * D];
        double r2 = 0.0;
        for (int k = 0; k < D; k++) r2 += (x[k] - 0.3) * (x[k] - 0.3);
        double *u = &U[(size_t)v * C];
        u[0] = std::tanh(20.0 * (x[0] - 0.5 + 0.2 * x[1])) + x[D - 1] * x[D - 1];
        u[1] = 1e3 * std::exp(-50.0 * r2);
        u[2] = 3.0 * x[0] - 1.0;
        if (C > 3) u[3] = std::sin(5.0 * x[D - 1] + x[0]);
    }
    const double w[4] = {1.0, 1e-3, 1.0, 0.75};
    double *d_U = nullptr;
    if (hipMalloc((void **)&d_U, U.size() * 8) != hipSuccess ||
        hipMemcpy(d_U, U.data(), U.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
        throw std::runtime_error("device copy of U failed");

    const std::string tag = D == 2 ? "2d" : "3d";
    const std::vector<double> g0 = grid_of(A.handle());
    // Huang's form, alpha solved and given
    const double alphas[2] = {0.0, 2.5};
    for (double alpha : alphas) {
        const std::string t = tag + (alpha == 0.0 ? "_solved" : "_given");
        double hostAlpha = -1.0;
        mmadmm_cxx::check(mmadmm_fields_monitor(D, nP, X.data(), nF, f.data(), C, U.data(), w, alpha, 1, &hostAlpha,
                                                nullptr, nullptr, M.data()));
        B.regridFromValues(M.data());
        const std::vector<double> gb = grid_of(B.handle());
        const double a1 = A.regridFromFieldsHuang(U.data(), C, w, alpha);
        const std::vector<double> g1 = grid_of(A.handle());
        const double a2 = A.regridFromFieldsHuang(d_U, C, w, alpha, true);
        const std::vector<double> g2 = grid_of(A.handle());
        report("alpha_host_array_" + t, a1 == hostAlpha && (alpha == 0.0 || a1 == alpha));
        report("alpha_device_array_" + t, a2 == hostAlpha);
        report("grid_host_array_" + t, same(g1, gb));
        report("grid_device_array_" + t, same(g2, gb));
        report("grid_changed_" + t, !same(g1, g0));
    }
    // the plain form, and the defaults of the normalised one (no weights, alpha solved)
    mmadmm_cxx::check(mmadmm_fields_monitor(D, nP, X.data(), nF, f.data(), C, U.data(), w, 40.0, 0, nullptr, nullptr,
                                            nullptr, M.data()));
    B.regridFromValues(M.data());
    const std::vector<double> gp = grid_of(B.handle());
    A.regridFromFields(U.data(), C, w, 40.0);
    report("grid_plain_host_array_" + tag, same(grid_of(A.handle()), gp));
    A.regridFromFields(d_U, C, w, 40.0, true);
    report("grid_plain_device_array_" + tag, same(grid_of(A.handle()), gp));
    double hostAlpha = -1.0;
    mmadmm_cxx::check(mmadmm_fields_monitor(D, nP, X.data(), nF, f.data(), C, U.data(), nullptr, 0.0, 1, &hostAlpha,
                                            nullptr, nullptr, M.data()));
    B.regridFromValues(M.data());
    const double ad = A.regridFromFieldsHuang(d_U, C, nullptr, 0.0, true);
    report("defaults_" + tag, A.regridFromFieldsHuang(U.data(), C) == hostAlpha && ad == hostAlpha &&
                                  same(grid_of(A.handle()), grid_of(B.handle())));
    (void)hipFree(d_U);

    auto refused = [&](auto call) {
        try {
            call();
        } catch (const mmadmm_cxx::Error &e) {
            return e.code == MMADMM_ERR_INVALID;
        }
        return false;
    };
    const double bad[4] = {1.0, -1.0, 1.0, 1.0};
    report("alpha_negative_refused_" + tag, refused([&] { A.regridFromFieldsHuang(U.data(), C, w, -1.0); }));
    report("alpha_zero_refused_plain_" + tag, refused([&] { A.regridFromFields(U.data(), C, w, 0.0); }));
    report("weight_refused_" + tag, refused([&] { A.regridFromFields(U.data(), C, bad, 1.0); }));
    report("count_refused_" + tag, refused([&] { A.regridFromFieldsHuang(U.data(), 33); }));
}

int main() {
    try {
        run<2>(6);
        run<3>(3);
    } catch (const std::exception &e) {
        printf("exception FAIL: %s\n", e.what());
        return 1;
    }
    return fails ? 1 : 0;
}
