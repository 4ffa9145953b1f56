// field_regrid_check.cpp -- MeshIntegrator<D>::regridFromField / regridFromValues (include/mmadmm/
// MeshIntegrator.h) against the C-ABI calls they mirror: two engines on the same mesh, one driven
// through the C++ class, one through mmadmm_regrid_field / mmadmm_regrid_values; the rebuilt
// monitor grids must be equal bit for bit.  Prints one "<name> ok|FAIL" line per check.
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
    Mesh<D> mesh(V, F, mask, &mon, 1, 1000.0, 0.0, 0.5, 0, false);
    MeshIntegrator<D> integ(0.025, mesh);
    const int nP = (int)V.rows();

    // the same problem through the plain C-ABI
    std::vector<double> xp = Mesh<D>::rowMajor(V);
    std::vector<int32_t> f = Mesh<D>::rowMajor(F), m(nP);
    for (int i = 0; i < nP; i++) m[i] = (int32_t)mask[i];
    mmadmm_params prm{};
    prm.dt = 0.025;
    prm.tau = 0.5;
    prm.rho = 1000.0;
    prm.device = -1;
    prm.nranks = 1;
    mmadmm_handle h = nullptr;
    mmadmm_cxx::check(mmadmm_create(D, nP, xp.data(), nullptr, (int)F.rows(), f.data(), m.data(), &prm,
                                    &mmadmm_cxx::monitor_trampoline<D>, &mon, &h));

    std::vector<double> u(nP);
    for (int v = 0; v < nP; v++) {
        const double *x = &xp[(size_t)v * D];
        u[v] = std::tanh(20.0 * (x[0] - 0.5 + 0.2 * x[1])) + x[D - 1] * x[D - 1];
    }
    const std::string tag = D == 2 ? "2d" : "3d";
    const std::vector<double> g0 = grid_of(h);
    integ.regridFromField(u.data(), 2.5);
    mmadmm_cxx::check(mmadmm_regrid_field(h, u.data(), 2.5));
    const std::vector<double> ga = grid_of(integ.handle()), gb = grid_of(h);
    report("field_grid_equal_" + tag, ga.size() == gb.size() && std::memcmp(ga.data(), gb.data(), ga.size() * 8) == 0);
    report("field_grid_changed_" + tag, ga.size() != g0.size() || std::memcmp(ga.data(), g0.data(), ga.size() * 8) != 0);

    std::vector<double> M((size_t)nP * D * D, 0.0);
    for (int v = 0; v < nP; v++)
        for (int i = 0; i < D; i++) M[(size_t)v * D * D + i * D + i] = 1.0 + 0.5 * xp[(size_t)v * D];
    integ.regridFromValues(M.data());
    mmadmm_cxx::check(mmadmm_regrid_values(h, M.data()));
    const std::vector<double> va = grid_of(integ.handle()), vb = grid_of(h);
    report("values_grid_equal_" + tag, va.size() == vb.size() && std::memcmp(va.data(), vb.data(), va.size() * 8) == 0);

    bool refused = false;
    try {
        integ.regridFromField(u.data(), 0.0);
    } catch (const mmadmm_cxx::Error &e) {
        refused = e.code == MMADMM_ERR_INVALID;
    }
    report("alpha_zero_refused_" + tag, refused);
    mmadmm_destroy(h);
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
