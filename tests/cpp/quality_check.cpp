// quality_check.cpp -- MeshIntegrator<D>::quality (include/mmadmm/MeshIntegrator.h), host and device
// flavours, against the C-ABI calls it mirrors: two engines on the same mesh take the same step,
// one driven through the C++ class, one through mmadmm_step / mmadmm_quality(_device); the measures
// must be equal bit for bit, and equal to the host-only mmadmm_mesh_quality.
// Prints one "<name> ok|FAIL" line per check.
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
class Bump : public MonitorFunction<D> {
public:
    void operator()(Eigen::Vector<double, D> &x, Eigen::Matrix<double, D, D> &M) override {
        double r2 = 0;
        for (int i = 0; i < D; i++) r2 += (x(i) - 0.4) * (x(i) - 0.4);
        M.setZero();
        for (int i = 0; i < D; i++) M(i, i) = 1.0 + 5.0 / (1.0 + 50.0 * r2);
    }
};

static int fails = 0;
static void report(const std::string &name, bool ok) {
    printf("%s %s\n", name.c_str(), ok ? "ok" : "FAIL");
    if (!ok) fails++;
}
static bool same(const std::vector<double> &a, const std::vector<double> &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0;
}
static void hip_ok(hipError_t e) {
    if (e != hipSuccess) throw std::runtime_error(hipGetErrorString(e));
}
static double *to_device(const std::vector<double> &v) {
    double *d = nullptr;
    hip_ok(hipMalloc((void **)&d, v.size() * sizeof(double)));
    hip_ok(hipMemcpy(d, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice));
    return d;
}
static std::vector<double> to_host(const double *d, size_t n) {
    std::vector<double> v(n);
    hip_ok(hipMemcpy(v.data(), d, n * sizeof(double), hipMemcpyDeviceToHost));
    return v;
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
    Bump<D> mon;
    Mesh<D> mesh(V, F, mask, &mon, 1, 1000.0, 0.0, 0.5, 0, false);
    MeshIntegrator<D> integ(0.025, mesh);
    const int nP = (int)V.rows(), nF = (int)F.rows();

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
    mmadmm_cxx::check(mmadmm_create(D, nP, xp.data(), nullptr, nF, f.data(), m.data(), &prm,
                                    &mmadmm_cxx::monitor_trampoline<D>, &mon, &h));
    integ.step(5, -1.0);
    double Ih = 0;
    int iters = 0;
    mmadmm_cxx::check(mmadmm_step(h, 5, -1.0, &Ih, &iters));

    // nodal tensors: the bump monitor at the initial positions, with a shear
    std::vector<double> M((size_t)nP * D * D, 0.0);
    for (int v = 0; v < nP; v++) {
        const double *x = &xp[(size_t)v * D];
        double r2 = 0;
        for (int i = 0; i < D; i++) r2 += (x[i] - 0.4) * (x[i] - 0.4);
        for (int i = 0; i < D; i++) M[(size_t)v * D * D + i * D + i] = 1.0 + 5.0 / (1.0 + 50.0 * r2);
        M[(size_t)v * D * D + 1] = M[(size_t)v * D * D + D] = 0.25 * x[0];
    }
    const std::string tag = D == 2 ? "2d" : "3d";
    std::vector<double> a((size_t)3 * nF, -1.0), b(a.size(), -2.0), c(a.size(), -3.0), sa(8, -1.0), sb(8, -2.0), sc(8, -3.0);
    integ.quality(MMADMM_QUALITY_VALUES, M.data(), a.data(), sa.data());
    mmadmm_cxx::check(mmadmm_quality(h, nullptr, MMADMM_QUALITY_VALUES, M.data(), b.data(), sb.data()));
    report("host_equal_" + tag, same(a, b) && same(sa, sb));
    std::vector<double> xnew((size_t)nP * D), Ehat((size_t)D * D);
    std::vector<int32_t> fe((size_t)nF * (D + 1));
    mmadmm_cxx::check(mmadmm_get(h, "points", xnew.data()));
    mmadmm_cxx::check(mmadmm_get(h, "Ehat", Ehat.data()));
    mmadmm_cxx::check(mmadmm_get_simplices(h, fe.data()));
    mmadmm_cxx::check(mmadmm_mesh_quality(D, nP, xnew.data(), nullptr, nF, fe.data(), Ehat.data(), M.data(), c.data(),
                                          sc.data()));
    report("host_equals_cpu_function_" + tag, same(a, c) && same(sa, sc));
    report("measures_sane_" + tag, sa[0] >= 1.0 && sa[1] >= 1.0 && sa[2] >= 1.0 - 1e-12 && sa[7] == 0.0 &&
                                       std::fabs(sa[6] - 1.0) <= 1e-12 && xnew != xp);

    double *dM = to_device(M), *dX = to_device(xnew), *dA = to_device(c), *dB = to_device(c);
    hip_ok(hipMemset(dA, 0, a.size() * sizeof(double)));
    hip_ok(hipMemset(dB, 0, a.size() * sizeof(double)));
    std::vector<double> da_s(8, -1.0), db_s(8, -2.0);
    integ.quality(MMADMM_QUALITY_VALUES, dM, dA, da_s.data(), dX, true);
    mmadmm_cxx::check(mmadmm_quality_device(h, nullptr, MMADMM_QUALITY_VALUES, dM, dB, db_s.data(), nullptr));
    const std::vector<double> da = to_host(dA, a.size()), db = to_host(dB, a.size());
    report("device_equal_" + tag, same(da, db) && same(da_s, db_s));
    report("device_equals_host_" + tag, same(da, a) && same(da_s, sa));
    for (double *q : {dM, dX, dA, dB}) hip_ok(hipFree(q));

    // the nodal monitor of the last rebuild: that of regridFromValues
    integ.regridFromValues(M.data());
    std::vector<double> sl(8, -1.0);
    integ.quality(MMADMM_QUALITY_LAST, nullptr, nullptr, sl.data());
    report("last_equals_values_" + tag, same(sl, sa));

    bool refused = false;
    try {
        integ.quality(MMADMM_QUALITY_VALUES, nullptr, a.data(), sa.data());
    } catch (const mmadmm_cxx::Error &e) {
        refused = e.code == MMADMM_ERR_INVALID;
    }
    report("values_without_tensors_refused_" + tag, refused);
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
