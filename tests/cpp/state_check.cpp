// state_check.cpp -- MeshIntegrator<D>::saveState / loadState (include/mmadmm/MeshIntegrator.h): the
// file, host-buffer and device-buffer flavours.  One integrator runs four steps; a second one saves
// after two, is destroyed, and three new ones load the file, the host blob and the device blob and
// finish: the points of every step, the energies and the Mesh's Vp must be equal bit for bit.  The
// three blobs must be the same bytes, and a blob of another dt refused with nothing changed.
// Prints one "<name> ok|FAIL" line per check.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
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
        for (int i = 0; i < D; i++) M(i, i) = 1.0 + 5.0 / (1.0 + 20.0 * r2);
    }
};

static int fails = 0;
static void report(const std::string &name, bool ok) {
    printf("%s %s\n", name.c_str(), ok ? "ok" : "FAIL");
    if (!ok) fails++;
}
static void hip_ok(hipError_t e) {
    if (e != hipSuccess) throw std::runtime_error(hipGetErrorString(e));
}
static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

template <int D>
struct Problem {
    Eigen::MatrixXd V;
    Eigen::MatrixXi F;
    std::vector<NodeType> mask;
    Bump<D> mon;
    std::unique_ptr<Mesh<D>> mesh;
    std::unique_ptr<MeshIntegrator<D>> integ;
    Problem(int n, double dt) {
        std::unordered_map<std::string, double> p{{"nx", (double)n}, {"ny", (double)n}, {"nz", (double)n}, {"xa", 0},
                                                  {"xb", 1},         {"ya", 0},         {"yb", 1},         {"za", 0},
                                                  {"zb", 1}};
        utils::generateUniformRectMesh<D>(p, &V, &F, &mask, NodeType::BOUNDARY_FIXED);
        mesh.reset(new Mesh<D>(V, F, mask, &mon, 1, 1000.0, 0.0, 0.5, 0, false));
        integ.reset(new MeshIntegrator<D>(dt, *mesh));
    }
    std::vector<double> points() {
        std::vector<double> x((size_t)V.rows() * D);
        mmadmm_cxx::check(mmadmm_get(integ->handle(), "points", x.data()));
        return x;
    }
    bool meshFollows() {  // the Mesh's Vp is the engine's points
        const std::vector<double> x = points(), v = Mesh<D>::rowMajor(*mesh->Vp);
        return x.size() == v.size() && std::memcmp(x.data(), v.data(), x.size() * sizeof(double)) == 0;
    }
};

struct Step {
    double Ih;
    std::vector<double> x;
};
template <int D>
static std::vector<Step> take(Problem<D> &p, int n) {
    std::vector<Step> out;
    for (int k = 0; k < n; k++) {
        const double Ih = p.integ->step(5, -1.0);
        out.push_back({Ih, p.points()});
    }
    return out;
}
static bool same_steps(const std::vector<Step> &a, const std::vector<Step> &b, size_t from) {
    if (a.size() + from != b.size()) return false;
    for (size_t k = 0; k < a.size(); k++)
        if (!same_bits(a[k].Ih, b[from + k].Ih) || a[k].x.size() != b[from + k].x.size() ||
            std::memcmp(a[k].x.data(), b[from + k].x.data(), a[k].x.size() * sizeof(double)) != 0)
            return false;
    return true;
}

template <int D>
static void run(int n, const std::string &dir) {
    const std::string tag = D == 2 ? "2d" : "3d", path = dir + "/state_check_" + tag + ".mmx";
    const double dt = 0.025;
    Problem<D> whole(n, dt);
    const std::vector<Step> want = take(whole, 4);

    std::vector<unsigned char> host, fromDev;
    void *dBlob = nullptr;
    long long bytes = 0;
    {
        Problem<D> saver(n, dt);
        take(saver, 2);
        bytes = saver.integ->stateBytes();
        host.resize((size_t)bytes);
        fromDev.resize((size_t)bytes);
        saver.integ->saveState(path.c_str());
        saver.integ->saveState(host.data(), bytes);
        hip_ok(hipMalloc(&dBlob, (size_t)bytes));
        saver.integ->saveState(dBlob, bytes, true);
        hip_ok(hipMemcpy(fromDev.data(), dBlob, (size_t)bytes, hipMemcpyDeviceToHost));
    }  // destroyed
    std::vector<unsigned char> filed((size_t)bytes);
    bool readOk = false;
    if (FILE *f = std::fopen(path.c_str(), "rb")) {
        readOk = std::fread(filed.data(), 1, filed.size(), f) == filed.size() && std::fgetc(f) == EOF;
        std::fclose(f);
    }
    report("three_blobs_equal_" + tag, readOk && host == filed && host == fromDev);
    mmadmm_state_header hd;
    report("info_" + tag, mmadmm_state_info(host.data(), bytes, &hd) == MMADMM_OK && hd.steps_taken == 2 &&
                              hd.dim == D && hd.nP == whole.V.rows() && hd.nF == whole.F.rows() && hd.hess_computed == 1);

    {
        Problem<D> p(n, dt);
        p.integ->loadState(path.c_str());
        report("file_counts_and_mesh_" + tag, p.integ->stepsTaken == 2 && p.meshFollows());
        report("file_continues_" + tag, same_steps(take(p, 2), want, 2) && p.integ->stepsTaken == 4);
    }
    {
        Problem<D> p(n, dt);
        p.integ->loadState(host.data(), bytes);
        report("host_continues_" + tag, p.integ->stepsTaken == 2 && p.meshFollows() && same_steps(take(p, 2), want, 2));
    }
    {
        Problem<D> p(n, dt);
        p.integ->loadState(dBlob, bytes, true);
        report("device_continues_" + tag, p.meshFollows() && same_steps(take(p, 2), want, 2));
    }
    hip_ok(hipFree(dBlob));
    {
        // another dt: refused by the fingerprint, and the integrator steps as one that never saw the call
        Problem<D> p(n, 0.0125), q(n, 0.0125);
        bool refused = false;
        try {
            p.integ->loadState(host.data(), bytes);
        } catch (const mmadmm_cxx::Error &e) {
            refused = e.code == MMADMM_ERR_INVALID && std::string(e.what()).find("fingerprint") != std::string::npos;
        }
        bool io = false;
        try {
            p.integ->loadState((dir + "/no_such_file.mmx").c_str());
        } catch (const mmadmm_cxx::Error &e) {
            io = e.code == MMADMM_ERR_IO;
        }
        report("other_dt_refused_" + tag, refused && io && p.integ->stepsTaken == 0);
        report("refusal_changes_nothing_" + tag, same_steps(take(p, 1), take(q, 1), 0));
    }
    std::remove(path.c_str());
}

int main(int argc, char **argv) {
    const std::string dir = argc > 1 ? argv[1] : ".";
    try {
        run<2>(6, dir);
        run<3>(3, dir);
    } catch (const std::exception &e) {
        printf("exception FAIL: %s\n", e.what());
        return 1;
    }
    return fails ? 1 : 0;
}
