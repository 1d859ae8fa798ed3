/* oracle/ref_front.cpp -- driver around the reference's OWN initRegistration_KSS and PCR_QM classes
 * (TEST INFRASTRUCTURE, NOT PRODUCT CODE).
 *
 * oracle/Makefile.ref compiles this file against the reference's initRegistrationKSS.hpp and
 * registrationMeasure.hpp, found through an -I path at build time (nothing of them is copied here), and the
 * stand-in PCL headers of oracle/ref_shim.  The binary, oracle/_ref/kss_ref_front, is what
 * tests/golden/make_ref_front.py records into tests/golden/ref_front.npz and what tests/test_ref_front_host.py
 * compares oracle/kss_oracle.c with, bit for bit.
 *
 *   kss_ref_front front IN OUT    IN : int64 ns, nt; double step; double S[3 ns]; double T[3 nt]
 *                                 OUT: int64 g, nl, ns, nra; then doubles:
 *                                      x/y/z_middle_S, x/y/z_middle, scale            (7)
 *                                      angle                                          (3)
 *                                      value[g][g][g]                                 (g^3)
 *                                      angleList                                      (3 nl)
 *                                      pointSource after initRegistration_init        (3 ns)
 *                                      initRegistration_Rotation(S)                   (3 ns)
 *                                      initRegistration_Rotation_Angle(S, angleList[i]), i < nra = min(3, nl)
 *                                      PCR_QM(initRegistration_Rotation(S), T)        (3)
 *   kss_ref_front qm IN OUT       IN : int64 na, nt; double A[3 na]; double T[3 nt]
 *                                 OUT: double MSE, RMSE, MAE
 *
 * The files are flat and in host byte order.  The reference's progress output to cout is discarded. */
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <iostream>
#include <math.h>
#include <memory>
#include <string>
#include <time.h>
#include <vector>

/* The error volume `value` is a private member.  Every standard header the two reference headers (and the
 * stand-ins) pull in is already included above, so this reaches no further than those two classes, in this
 * translation unit only. */
#define private public
#include <initRegistrationKSS.hpp>
#include <registrationMeasure.hpp>
#undef private

typedef std::vector<std::vector<double> > Cloud;

static void die(const char *what) {
    std::fprintf(stderr, "kss_ref_front: %s\n", what);
    std::exit(2);
}

static void read_exact(std::FILE *f, void *p, size_t bytes) {
    if (bytes && std::fread(p, 1, bytes, f) != bytes) die("short input file");
}

static Cloud read_cloud(std::FILE *f, int64_t n) {
    if (n < 0 || n > (int64_t)1 << 24) die("bad cloud size");
    std::vector<double> flat(3 * (size_t)n);
    read_exact(f, flat.data(), flat.size() * sizeof(double));
    Cloud c((size_t)n, std::vector<double>(3));
    for (size_t i = 0; i < (size_t)n; i++)
        for (int k = 0; k < 3; k++) c[i][k] = flat[3 * i + k];
    return c;
}

static void put(std::vector<double> &out, const Cloud &c) {
    for (size_t i = 0; i < c.size(); i++) {
        if (c[i].size() != 3) die("a point without three coordinates");
        out.insert(out.end(), c[i].begin(), c[i].end());
    }
}

static void write_all(const char *path, const std::vector<int64_t> &head, const std::vector<double> &body) {
    std::FILE *f = std::fopen(path, "wb");
    if (!f) die("cannot open the output file");
    if ((head.size() && std::fwrite(head.data(), sizeof(int64_t), head.size(), f) != head.size()) ||
        (body.size() && std::fwrite(body.data(), sizeof(double), body.size(), f) != body.size()) || std::fclose(f) != 0)
        die("cannot write the output file");
}

static std::vector<double> run_qm(const Cloud &a, const Cloud &t) {
    PCR_QM qm;
    qm.PCR_QM_init(a, t);
    std::vector<double> r = qm.PCR_QM_ReturnResult();
    if (r.size() != 3) die("PCR_QM returned no triple");
    return r;
}

int main(int argc, char **argv) {
    if (argc != 4) die("usage: kss_ref_front front|qm IN OUT");
    std::cout.setstate(std::ios_base::failbit);   /* the reference narrates to cout */
    std::FILE *f = std::fopen(argv[2], "rb");
    if (!f) die("cannot open the input file");
    int64_t n[2];
    read_exact(f, n, sizeof n);
    std::vector<double> out;

    if (std::strcmp(argv[1], "qm") == 0) {
        Cloud A = read_cloud(f, n[0]), T = read_cloud(f, n[1]);
        std::fclose(f);
        out = run_qm(A, T);
        write_all(argv[3], std::vector<int64_t>(), out);
        return 0;
    }
    if (std::strcmp(argv[1], "front") != 0) die("unknown mode");

    double step;
    read_exact(f, &step, sizeof step);
    Cloud S = read_cloud(f, n[0]), T = read_cloud(f, n[1]);
    std::fclose(f);

    initRegistration_KSS ir;
    ir.initRegistration_init(S, T, step);

    const size_t g = ir.value.size();
    for (size_t i = 0; i < g; i++) {
        if (ir.value[i].size() != g) die("the error volume is not a cube");
        for (size_t j = 0; j < g; j++)
            if (ir.value[i][j].size() != g) die("the error volume is not a cube");
    }
    if ((size_t)ir.irange != g || (size_t)ir.jrange != g || (size_t)ir.krange != g) die("ranges differ from the volume");
    if (ir.angle.size() != 3) die("angle is no triple");
    const size_t nl = ir.angleList.size();
    const size_t nra = std::min<size_t>(3, nl);

    out.push_back(ir.x_middle_S); out.push_back(ir.y_middle_S); out.push_back(ir.z_middle_S);
    out.push_back(ir.x_middle); out.push_back(ir.y_middle); out.push_back(ir.z_middle);
    out.push_back(ir.scale);
    out.insert(out.end(), ir.angle.begin(), ir.angle.end());
    for (size_t i = 0; i < g; i++)
        for (size_t j = 0; j < g; j++) out.insert(out.end(), ir.value[i][j].begin(), ir.value[i][j].end());
    put(out, ir.angleList);
    put(out, ir.pointSource);
    Cloud posed = ir.initRegistration_Rotation(S);
    put(out, posed);
    for (size_t i = 0; i < nra; i++) put(out, ir.initRegistration_Rotation_Angle(S, ir.angleList[i]));
    std::vector<double> qm = run_qm(posed, T);
    out.insert(out.end(), qm.begin(), qm.end());

    std::vector<int64_t> head;
    head.push_back((int64_t)g); head.push_back((int64_t)nl); head.push_back((int64_t)S.size()); head.push_back((int64_t)nra);
    write_all(argv[3], head, out);
    return 0;
}
