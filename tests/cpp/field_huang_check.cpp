// field_huang_check.cpp -- MeshIntegrator<D>::regridFromFieldHuang (include/mmadmm/MeshIntegrator.h)
// with a host array and with a device array, alpha solved and given, against the host-only
// mmadmm_field_monitor_huang followed by regridFromValues on a second engine: the alphas and the
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
    std::vector<double> X((size_t)nP * D), u(nP), M((size_t)nP * D * D);
    std::vector<int32_t> f((size_t)nF * (D + 1));
    mmadmm_cxx::check(mmadmm_get(A.handle(), "points", X.data()));
    mmadmm_cxx::check(mmadmm_get_simplices(A.handle(), f.data()));
    for (int v = 0; v < nP; v++) {
        const double *x = &X[(size_t)v * D];
        u[v] = std::tanh(20.0 * (x[0] - 0.5 + 0.2 * x[1])) + x[D - 1] * x[D - 1];
    }
    double *d_u = nullptr;
    if (hipMalloc((void **)&d_u, (size_t)nP * 8) != hipSuccess ||
        hipMemcpy(d_u, u.data(), (size_t)nP * 8, hipMemcpyHostToDevice) != hipSuccess)
        throw std::runtime_error("device copy of u failed");

    const std::string tag = D == 2 ? "2d" : "3d";
    const std::vector<double> g0 = grid_of(A.handle());
    const double alphas[2] = {0.0, 2.5};
    for (double alpha : alphas) {
        const std::string t = tag + (alpha == 0.0 ? "_solved" : "_given");
        double hostAlpha = -1.0;
        mmadmm_cxx::check(mmadmm_field_monitor_huang(D, nP, X.data(), nF, f.data(), u.data(), alpha, &hostAlpha, nullptr,
                                                     M.data()));
        B.regridFromValues(M.data());
        const std::vector<double> gb = grid_of(B.handle());
        const double a1 = A.regridFromFieldHuang(u.data(), alpha);
        const std::vector<double> g1 = grid_of(A.handle());
        const double a2 = A.regridFromFieldHuang(d_u, alpha, true);
        const std::vector<double> g2 = grid_of(A.handle());
        report("alpha_host_array_" + t, a1 == hostAlpha && (alpha == 0.0 || a1 == alpha));
        report("alpha_device_array_" + t, a2 == hostAlpha);
        report("grid_host_array_" + t, same(g1, gb));
        report("grid_device_array_" + t, same(g2, gb));
        report("grid_changed_" + t, !same(g1, g0));
    }
    (void)hipFree(d_u);

    bool refused = false;
    try {
        A.regridFromFieldHuang(u.data(), -1.0);
    } catch (const mmadmm_cxx::Error &e) {
        refused = e.code == MMADMM_ERR_INVALID;
    }
    report("alpha_negative_refused_" + tag, refused);
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
