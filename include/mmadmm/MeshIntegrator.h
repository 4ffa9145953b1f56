// MeshIntegrator.h -- the reference's MeshIntegrator<D> (src/MeshIntegrator.h:12-51) over the
// C-ABI of libmmadmm.so.
//
//   MeshIntegrator(double dt, Mesh<D> &a)      src/MeshIntegrator.cpp:15-62 -> mmadmm_create
//   double step(int nIters, double tol)         src/MeshIntegrator.cpp:101-191 -> mmadmm_step
//   double eulerStep(double tol)                src/MeshIntegrator.cpp:87-94 -> mmadmm_euler_step
//   double backwardsEulerStep(double dt, double tol)
//                                               src/MeshIntegrator.cpp:68-76 -> mmadmm_backward_euler_step
//   double getEnergy()                          src/MeshIntegrator.cpp:79-81 -> mmadmm_energy
//   void done()                                 src/MeshIntegrator.cpp:193-196 -> mmadmm_done
//   void outputX / outputZ(const char *fname)   src/MeshIntegrator.cpp:218-246
//   double proxTime, predTime, multTime, cgTime public timers (wall seconds; the device does the
//                                               whole step, so proxTime holds step() time)
// step() writes the positions back into the Mesh's Xp after every step, as the reference's
// updateAfterStep does; eulerStep/backwardsEulerStep leave Xp to done(), as in the reference.
// One integrator per Mesh (the reference's is not re-entrant either).
#ifndef SOLVER_H
#define SOLVER_H

#include <chrono>
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

#include "Mesh.h"

using namespace std;

template <int D>
class MeshIntegrator {
public:
    MeshIntegrator(double dt, Mesh<D> &a) : a(&a), dt(dt), dtPrev(dt) {
        if (a.h_) throw mmadmm_cxx::Error(MMADMM_ERR_INVALID, "MeshIntegrator: the Mesh already has an integrator");
        std::vector<double> xp = Mesh<D>::rowMajor(*a.Vp), xc;
        if (a.compMesh) xc = Mesh<D>::rowMajor(*a.Vc);
        std::vector<int32_t> f = Mesh<D>::rowMajor(*a.F);
        const int nP = (int)a.Vp->rows();
        std::vector<int32_t> mask(nP);
        for (int i = 0; i < nP; i++) mask[i] = (int32_t)a.boundaryMask->at(i);
        mmadmm_params p{};
        p.dt = dt;
        p.tau = a.tau;
        p.rho = a.rho;
        p.grad_use = a.gradUse ? 1 : 0;
        p.device = -1;
        p.rank = 0;
        p.nranks = 1;
        mmadmm_cxx::check(mmadmm_create(D, nP, xp.data(), a.compMesh ? xc.data() : nullptr, (int)a.F->rows(), f.data(),
                                        mask.data(), &p, &mmadmm_cxx::monitor_trampoline<D>, a.Mon, &a.h_));
        h_ = a.h_;
    }
    ~MeshIntegrator() {
        if (h_) mmadmm_destroy(h_);
        if (a) a->h_ = nullptr;
    }
    MeshIntegrator(const MeshIntegrator &) = delete;
    MeshIntegrator &operator=(const MeshIntegrator &) = delete;

    double step(int nIters, double tol) {
        const auto t0 = std::chrono::steady_clock::now();
        double Ih = 0;
        int iters = 0;
        mmadmm_cxx::check(mmadmm_step(h_, nIters, tol, &Ih, &iters));
        a->updateAfterStep();
        proxTime += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        stepsTaken++;
        energyCur = Ih;
        return Ih;
    }
    double eulerStep(double tol) {
        (void)tol;
        double Ih = 0;
        mmadmm_cxx::check(mmadmm_euler_step(h_, &Ih));
        stepsTaken++;
        return Ih;
    }
    double backwardsEulerStep(double dtStep, double tol) {
        double Ih = 0;
        int newton = 0;
        mmadmm_cxx::check(mmadmm_backward_euler_step(h_, dtStep, tol, &Ih, &newton));
        stepsTaken++;
        return Ih;
    }
    // the reference's commented Mesh<D>::setUp hook (src/Mesh.cpp:1006-1014): rebuild the monitor
    // grid from the current mesh at the start of every step (no reference counterpart; off by default)
    void setTimeVarying(bool on) { mmadmm_cxx::check(mmadmm_set_regrid(h_, on ? 1 : 0)); }
    // the monitor from the caller's arrays at the current vertices (no reference counterpart): nP x D*D
    // row-major tensors, or a nodal scalar field u (nP values) whose recovered Hessian H gives
    // M = I + |H| / alpha.  onDevice: the array is in device memory and ready (include/mmadmm.h:
    // mmadmm_regrid_values / mmadmm_regrid_field and their _device forms)
    void regridFromValues(const double *M, bool onDevice = false) {
        mmadmm_cxx::check(onDevice ? mmadmm_regrid_values_device(h_, M, nullptr) : mmadmm_regrid_values(h_, M));
    }
    void regridFromField(const double *u, double alpha, bool onDevice = false) {
        mmadmm_cxx::check(onDevice ? mmadmm_regrid_field_device(h_, u, alpha, nullptr)
                                   : mmadmm_regrid_field(h_, u, alpha));
    }
    // Huang's normalised monitor M = det(I + |H| / alpha)^(-1/(D+4)) (I + |H| / alpha) of the field u;
    // alpha 0: solved on the device from the equidistribution equation.  Returns the alpha used, to
    // be passed to later calls (include/mmadmm.h: mmadmm_regrid_field_huang and its _device form)
    double regridFromFieldHuang(const double *u, double alpha = 0.0, bool onDevice = false) {
        double used = 0.0;
        mmadmm_cxx::check(onDevice ? mmadmm_regrid_field_huang_device(h_, u, alpha, nullptr, &used)
                                   : mmadmm_regrid_field_huang(h_, u, alpha, &used));
        return used;
    }
    // the same two monitors from C components per node (U nP x C row-major, as transferField carries
    // them): the metric is the weighted sum of the components' absolute Hessians, w C host weights
    // (nullptr: all 1) whatever onDevice says (include/mmadmm.h: mmadmm_regrid_fields(_huang) and
    // their _device forms)
    void regridFromFields(const double *U, int C, const double *w, double alpha, bool onDevice = false) {
        mmadmm_cxx::check(onDevice ? mmadmm_regrid_fields_device(h_, C, U, w, alpha, nullptr)
                                   : mmadmm_regrid_fields(h_, C, U, w, alpha));
    }
    double regridFromFieldsHuang(const double *U, int C, const double *w = nullptr, double alpha = 0.0,
                                 bool onDevice = false) {
        double used = 0.0;
        mmadmm_cxx::check(onDevice ? mmadmm_regrid_fields_huang_device(h_, C, U, w, alpha, nullptr, &used)
                                   : mmadmm_regrid_fields_huang(h_, C, U, w, alpha, &used));
        return used;
    }
    // the caller's nodal field (C components per node, nP x C row-major) carried from the node
    // positions Xold (nP x D row-major, e.g. those before step()) to the current ones, piecewise
    // linearly on the old mesh (no reference counterpart; include/mmadmm.h: mmadmm_transfer and
    // mmadmm_transfer_device).  onDevice: all three arrays are in device memory and ready
    void transferField(const double *Xold, int C, const double *uold, double *unew, bool onDevice = false) {
        mmadmm_cxx::check(onDevice ? mmadmm_transfer_device(h_, Xold, nullptr, C, uold, unew, nullptr, nullptr, nullptr)
                                   : mmadmm_transfer(h_, Xold, nullptr, C, uold, unew, nullptr, nullptr));
    }
    // Nodal fields at arbitrary points (no reference counterpart; include/mmadmm.h: mmadmm_locator_build
    // and mmadmm_sample).  buildLocator: the cell locator over the simplices at the node positions X
    // (nP x D row-major; nullptr: the current points), automatic cells; it keeps its own copy of X.
    // sampleField: u (nP x C row-major) evaluated piecewise linearly at the nQ points Q (nQ x D) into
    // out (nQ x C); a point no cell locates is NaN.  onDevice: the arrays are in device memory and ready
    void buildLocator(const double *X = nullptr, bool onDevice = false) {
        mmadmm_cxx::check(onDevice ? mmadmm_locator_build_device(h_, X, nullptr, nullptr)
                                   : mmadmm_locator_build(h_, X, nullptr));
    }
    void sampleField(int nQ, const double *Q, int C, const double *u, double *out, bool onDevice = false) {
        mmadmm_cxx::check(onDevice ? mmadmm_sample_device(h_, nQ, Q, C, u, out, nullptr, nullptr, nullptr)
                                   : mmadmm_sample(h_, nQ, Q, C, u, out, nullptr, nullptr));
    }
    // Huang's geometry, alignment and equidistribution measures of the current mesh (X null) or of the
    // candidate positions X (nP x D row-major) against the monitor `source`: MMADMM_QUALITY_IDENTITY,
    // _VALUES (M: nP x D*D nodal tensors) or _LAST (the nodal monitor of the last grid rebuild, e.g. of
    // regridFromFieldHuang).  q (3 x nF component-major: Q_geo, Q_ali, Q_eq) and summary (8 host
    // doubles) may each be null, not both (no reference counterpart; include/mmadmm.h: mmadmm_quality
    // and mmadmm_quality_device).  onDevice: X, M and q are in device memory and ready
    void quality(int source, const double *M, double *q, double *summary, const double *X = nullptr,
                 bool onDevice = false) {
        mmadmm_cxx::check(onDevice ? mmadmm_quality_device(h_, X, source, M, q, summary, nullptr)
                                   : mmadmm_quality(h_, X, source, M, q, summary));
    }
    // BOUNDARY_FREE nodes slide on the boundary: every step() ends by projecting them onto the boundary
    // surface frozen at the first setBoundarySliding(true), on the device -- the reference's
    // Mesh<D>::projectOntoBoundary, whose call in updateAfterStep is commented out (src/Mesh.cpp:1020-1026).
    // Off by default.  projectOntoBoundary projects the caller's positions X (nP x D row-major, in place)
    // with the engine's anchors; onDevice: X is in device memory and ready (include/mmadmm.h:
    // mmadmm_set_boundary_slide, mmadmm_project_boundary and its _device form)
    void setBoundarySliding(bool on) { mmadmm_cxx::check(mmadmm_set_boundary_slide(h_, on ? 1 : 0)); }
    void projectOntoBoundary(double *X, bool onDevice = false) {
        mmadmm_cxx::check(onDevice ? mmadmm_project_boundary_device(h_, X, nullptr, nullptr, nullptr)
                                   : mmadmm_project_boundary(h_, X, nullptr, nullptr));
    }
    // The engine's whole state as one blob (no reference counterpart: the reference's FromFile restart
    // keeps the points alone; include/mmadmm.h: mmadmm_state_*).  saveState(path) writes a
    // checkpoint; loadState(path) into an integrator created from the same mesh, monitor, dt, tau and
    // rho continues the saved run bit for bit (stepsTaken and the Mesh's Vp follow).  The buffer
    // flavours are the snapshot to roll back to after a failed step: stateBytes() bytes, in host memory
    // or (onDevice) in device memory, 8-byte aligned and ready; after a device load stepsTaken, this
    // class's own count, is left to the caller (the header is in device memory).  A blob that does
    // not fit this integrator is refused (mmadmm_cxx::Error, MMADMM_ERR_INVALID) and changes nothing
    long long stateBytes() {
        long long n = 0;
        mmadmm_cxx::check(mmadmm_state_bytes(h_, &n));
        return n;
    }
    void saveState(const char *path) { mmadmm_cxx::check(mmadmm_state_write_file(h_, path)); }
    void saveState(void *buf, long long cap, bool onDevice = false) {
        mmadmm_cxx::check(onDevice ? mmadmm_state_save_device(h_, buf, cap, nullptr) : mmadmm_state_save(h_, buf, cap));
    }
    void loadState(const char *path) {
        mmadmm_cxx::check(mmadmm_state_read_file(h_, path));
        unsigned char head[512] = {0};
        if (FILE *f = std::fopen(path, "rb")) {
            const size_t got = std::fread(head, 1, sizeof head, f);
            std::fclose(f);
            afterLoad(got == sizeof head ? head : nullptr);
        } else {
            afterLoad(nullptr);
        }
    }
    void loadState(const void *buf, long long bytes, bool onDevice = false) {
        mmadmm_cxx::check(onDevice ? mmadmm_state_load_device(h_, buf, bytes, nullptr)
                                   : mmadmm_state_load(h_, buf, bytes));
        afterLoad(onDevice ? nullptr : buf);
    }
    // the engine behind this integrator, for the C-ABI calls the reference's class has no name for
    mmadmm_handle handle() const { return h_; }

    double getEnergy() {
        double E = 0;
        mmadmm_cxx::check(mmadmm_energy(h_, &E));
        return E;
    }
    void done() {
        mmadmm_cxx::check(mmadmm_done(h_));
        a->updateAfterStep();
    }
    void outputX(const char *fname) { output("x", fname); }
    void outputZ(const char *fname) { output("z", fname); }

    double proxTime = 0;
    double multTime = 0;
    double cgTime = 0;
    double predTime = 0;
    Mesh<D> *a;
    double dt;
    double dtPrev;
    double energyCur = INFINITY;
    int stepsTaken = 0;

private:
    mmadmm_handle h_ = nullptr;

    // after a load: the Mesh's Vp, and this class's step count from the blob's header (head: its 512
    // bytes in host memory; null for a device blob, whose count stays the caller's to set)
    void afterLoad(const void *head) {
        mmadmm_state_header hd;
        if (head && mmadmm_state_info(head, 512, &hd) == MMADMM_OK) stepsTaken = (int)hd.steps_taken;
        a->updateAfterStep();
    }

    void output(const char *what, const char *fname) {
        int nP = 0, nF = 0, rows = 0;
        mmadmm_cxx::check(mmadmm_sizes(h_, &nP, &nF, &rows));
        const size_t n = (what[0] == 'x') ? (size_t)nP * D : (size_t)nF * D * (D + 1);
        std::vector<double> v(n);
        mmadmm_cxx::check(mmadmm_get(h_, what, v.data()));
        mmadmm_cxx::check(mmadmm_write_points(fname, D, (int)(n / D), v.data()));
    }
};

#endif
