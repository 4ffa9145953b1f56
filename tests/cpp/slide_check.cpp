// slide_check.cpp -- MeshIntegrator<D>::setBoundarySliding / projectOntoBoundary (include/mmadmm/
// MeshIntegrator.h), host and device flavours, against the C-ABI calls they mirror: two engines on
// the same BOUNDARY_FREE mesh take the same step with sliding on, one driven through the C++ class,
// one through mmadmm_set_boundary_slide / mmadmm_step / mmadmm_project_boundary(_device); the points
// and the projected positions must be equal bit for bit, and equal to the host-only
// mmadmm_boundary_project_field.  Prints one "<name> ok|FAIL" line per check.
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
        for (int i = 0; i < D; i++) r2 += (x(i) - 0.5) * (x(i) - 0.5);
        M.setZero();
        for (int i = 0; i < D; i++) M(i, i) = 1.0 + 20.0 / (1.0 + 20.0 * r2);
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
    utils::generateUniformRectMesh<D>(p, &V, &F, &mask, NodeType::BOUNDARY_FREE);
    Bump<D> mon;
    // rho = 10: a mesh with BOUNDARY_FREE nodes inverts an element in its first prox at the suite's usual 1000
    Mesh<D> mesh(V, F, mask, &mon, 1, 10.0, 0.0, 0.5, 0, false);
    MeshIntegrator<D> integ(0.025, mesh);
    const int nP = (int)V.rows(), nF = (int)F.rows();

    // the same problem through the plain C-ABI
    std::vector<double> xp = Mesh<D>::rowMajor(V);
    std::vector<int32_t> f = Mesh<D>::rowMajor(F), m(nP);
    for (int i = 0; i < nP; i++) m[i] = (int32_t)mask[i];
    mmadmm_params prm{};
    prm.dt = 0.025;
    prm.tau = 0.5;
    prm.rho = 10.0;
    prm.device = -1;
    prm.nranks = 1;
    mmadmm_handle h = nullptr;
    mmadmm_cxx::check(mmadmm_create(D, nP, xp.data(), nullptr, nF, f.data(), m.data(), &prm,
                                    &mmadmm_cxx::monitor_trampoline<D>, &mon, &h));
    integ.setBoundarySliding(true);
    mmadmm_cxx::check(mmadmm_set_boundary_slide(h, 1));
    integ.step(5, -1.0);
    double Ih = 0;
    int iters = 0;
    mmadmm_cxx::check(mmadmm_step(h, 5, -1.0, &Ih, &iters));
    const std::string tag = D == 2 ? "2d" : "3d";
    std::vector<double> pa((size_t)nP * D), pb(pa.size());
    mmadmm_cxx::check(mmadmm_get(integ.handle(), "points", pa.data()));
    mmadmm_cxx::check(mmadmm_get(h, "points", pb.data()));
    int ca[5] = {0}, cb[5] = {0};
    double ma = 0, mb = 0;
    mmadmm_cxx::check(mmadmm_slide_counts(integ.handle(), ca, &ma));
    mmadmm_cxx::check(mmadmm_slide_counts(h, cb, &mb));
    report("step_equal_" + tag, same(pa, pb) && std::memcmp(ca, cb, sizeof ca) == 0 && ma == mb);
    report("some_node_slid_" + tag, ca[1] + ca[2] >= 1 && ca[3] == 0 && ma > 0.0 && !same(pa, xp));

    // the caller's own positions: every node pushed off, the anchors as the step left them
    int nS = 0;
    mmadmm_cxx::check(mmadmm_boundary_info(h, nullptr, &nS, nullptr, nullptr, nullptr));
    std::vector<int32_t> ids(nS), anc(nS), anchor(nP);
    mmadmm_cxx::check(mmadmm_boundary_info(h, nullptr, nullptr, nullptr, ids.data(), anc.data()));
    for (int v = 0; v < nP; v++) anchor[v] = v;
    for (int i = 0; i < nS; i++) anchor[ids[i]] = anc[i];
    std::vector<double> X(pa);
    for (int v = 0; v < nP; v++)
        for (int k = 0; k < D; k++) X[(size_t)v * D + k] += 0.3 / n * std::sin(1.0 + 3.0 * v + k);
    std::vector<double> a(X), b(X), c(X);
    std::vector<int32_t> fe((size_t)nF * (D + 1));
    mmadmm_cxx::check(mmadmm_get_simplices(h, fe.data()));
    mmadmm_cxx::check(mmadmm_boundary_project_field(D, nP, xp.data(), nF, fe.data(), m.data(), anchor.data(), c.data(),
                                                    nullptr, nullptr));
    double *dA = to_device(X), *dB = to_device(X);
    // each engine's anchors advance with a call: the device flavour starts from the step's anchors,
    // the host flavour below from those this call leaves (read back for the reference)
    integ.projectOntoBoundary(dA, true);
    mmadmm_cxx::check(mmadmm_project_boundary_device(h, dB, nullptr, nullptr, nullptr));
    const std::vector<double> da = to_host(dA, X.size()), db = to_host(dB, X.size());
    report("device_equal_" + tag, same(da, db));
    report("device_equals_cpu_function_" + tag, same(da, c) && !same(da, X));
    for (double *q : {dA, dB}) hip_ok(hipFree(q));

    std::vector<int32_t> anchor2(anchor);  // the anchors after that call
    mmadmm_cxx::check(mmadmm_boundary_info(h, nullptr, nullptr, nullptr, nullptr, anc.data()));
    for (int i = 0; i < nS; i++) anchor2[ids[i]] = anc[i];
    std::vector<double> c2(X);
    mmadmm_cxx::check(mmadmm_boundary_project_field(D, nP, xp.data(), nF, fe.data(), m.data(), anchor2.data(), c2.data(),
                                                    nullptr, nullptr));
    integ.projectOntoBoundary(a.data());
    mmadmm_cxx::check(mmadmm_project_boundary(h, b.data(), nullptr, nullptr));
    report("host_equal_" + tag, same(a, b));
    report("host_equals_cpu_function_" + tag, same(a, c2));

    bool refused = false;
    try {
        integ.projectOntoBoundary(nullptr);
    } catch (const mmadmm_cxx::Error &e) {
        refused = e.code == MMADMM_ERR_INVALID;
    }
    report("null_refused_" + tag, refused);
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
