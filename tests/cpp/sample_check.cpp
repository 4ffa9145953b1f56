// sample_check.cpp -- MeshIntegrator<D>::buildLocator / sampleField (include/mmadmm/MeshIntegrator.h),
// host and device flavours, against the C-ABI calls they mirror: two engines on the same mesh take the
// same step, one driven through the C++ class, one through mmadmm_step / mmadmm_locator_build /
// mmadmm_sample(_device); the sampled fields must be equal bit for bit, and equal to the host-only
// mmadmm_sample_field.  Prints one "<name> ok|FAIL" line per check.
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
    const int nP = (int)V.rows(), nF = (int)F.rows(), C = 2;

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

    std::vector<double> xnew((size_t)nP * D);
    std::vector<int32_t> fe((size_t)nF * (D + 1));
    mmadmm_cxx::check(mmadmm_get(h, "points", xnew.data()));
    mmadmm_cxx::check(mmadmm_get_simplices(h, fe.data()));
    std::vector<double> u((size_t)nP * C);
    for (int v = 0; v < nP; v++) {
        const double *x = &xnew[(size_t)v * D];
        u[(size_t)v * C] = std::tanh(20.0 * (x[0] - 0.5 + 0.2 * x[1])) + x[D - 1] * x[D - 1];
        u[(size_t)v * C + 1] = 1.0 + x[0] * x[1];
    }
    // the original (unmoved) node positions, every simplex centroid of the moved mesh, one point off the mesh
    std::vector<double> Q(xp);
    for (int s = 0; s < nF; s++)
        for (int k = 0; k < D; k++) {
            double c = 0;
            for (int j = 0; j < D + 1; j++) c += xnew[(size_t)fe[(size_t)s * (D + 1) + j] * D + k];
            Q.push_back(c / (D + 1));
        }
    for (int k = 0; k < D; k++) Q.push_back(k == 0 ? 1.5 : 0.3);
    const int nQ = (int)Q.size() / D;

    const std::string tag = D == 2 ? "2d" : "3d";
    std::vector<double> a((size_t)nQ * C, -1.0), b(a.size(), -2.0), c(a.size(), -3.0);
    integ.buildLocator();
    integ.sampleField(nQ, Q.data(), C, u.data(), a.data());
    int counts[3] = {0, 0, 0};
    mmadmm_cxx::check(mmadmm_locator_build(h, nullptr, nullptr));
    mmadmm_cxx::check(mmadmm_sample(h, nQ, Q.data(), C, u.data(), b.data(), nullptr, counts));
    report("host_equal_" + tag, same(a, b));
    report("counts_" + tag, counts[0] == nQ - 1 && counts[1] == 1 && counts[2] == 0);
    mmadmm_cxx::check(mmadmm_sample_field(D, nP, xnew.data(), nF, fe.data(), nullptr, nQ, Q.data(), C, u.data(), c.data(),
                                          nullptr, nullptr));
    report("host_equals_cpu_function_" + tag, same(a, c));

    double *dX = to_device(xnew), *dQ = to_device(Q), *dU = to_device(u), *dA = to_device(c), *dB = to_device(c);
    hip_ok(hipMemset(dA, 0, a.size() * sizeof(double)));
    hip_ok(hipMemset(dB, 0, a.size() * sizeof(double)));
    integ.buildLocator(dX, true);
    integ.sampleField(nQ, dQ, C, dU, dA, true);
    mmadmm_cxx::check(mmadmm_locator_build_device(h, dX, nullptr, nullptr));
    mmadmm_cxx::check(mmadmm_sample_device(h, nQ, dQ, C, dU, dB, nullptr, nullptr, nullptr));
    const std::vector<double> da = to_host(dA, a.size()), db = to_host(dB, a.size());
    report("device_equal_" + tag, same(da, db));
    report("device_equals_host_" + tag, same(da, a));
    for (double *q : {dX, dQ, dU, dA, dB}) hip_ok(hipFree(q));

    bool refused = false;
    try {
        integ.sampleField(nQ, Q.data(), 0, u.data(), a.data());
    } catch (const mmadmm_cxx::Error &e) {
        refused = e.code == MMADMM_ERR_INVALID;
    }
    report("no_components_refused_" + tag, refused);
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
