// GPU test of arma::interp2's method strings in include/mi355_arma.hpp: mi355::interp2(X, Y, Z, XI, YI, ZI, method, extrap)
// with "nearest", "linear" and an unknown string (which must throw std::invalid_argument), and a double, an integer and
// no seventh argument still reaching the linear overload.  Writes the inputs and results as raw doubles so that the
// Python test can compare them with its numpy references bit for bit.
//   arma_interp2_nearest_test OUT_DIR
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>

#include "mi355_arma.hpp"

static void dump(const std::string& path, const double* p, size_t n)
{
    FILE* fp = std::fopen(path.c_str(), "wb");
    std::fwrite(p, sizeof(double), n, fp);
    std::fclose(fp);
}
static void dump(const std::string& path, const arma::vec& v) { dump(path, v.memptr(), v.n_elem); }
static void dump(const std::string& path, const arma::mat& m) { dump(path, m.memptr(), m.n_elem); }

int main(int argc, char** argv)
{
    const std::string out = argc > 1 ? argv[1] : ".";
    const arma::uword nx = 23, ny = 17, nxi = 131, nyi = 301;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    arma::vec X(nx), Y(ny), XI(nxi), YI(nyi);
    arma::mat Z(ny, nx);
    // nodes on the grid of 1/8: every cell midpoint is an exact tie
    for (arma::uword j = 0; j < nx; ++j) X(j) = -2.0 + 0.125 * (double)(j * (j + 3) / 2);
    for (arma::uword i = 0; i < ny; ++i) Y(i) = 1.0 + 0.125 * (double)(i * (i + 5) / 2);
    for (arma::uword j = 0; j < nx; ++j)
        for (arma::uword i = 0; i < ny; ++i) Z(i, j) = 1000.0 * (double)(j + 1) + (double)(i + 1);      // encodes (i, j)
    Z(3, 4) = inf; Z(4, 4) = -inf; Z(7, 9) = nan; Z(0, 0) = -0.0; Z(ny - 1, nx - 1) = std::numeric_limits<double>::denorm_min(); Z(8, 2) = -0.0;
    unsigned long long s = 31;
    auto u = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * 0x1.0p-53; };
    for (arma::uword j = 0; j < nxi; ++j) XI(j) = u() * (X(nx - 1) - X(0) + 0.6) + X(0) - 0.3;   // unsorted, some out of range
    for (arma::uword i = 0; i < nyi; ++i) YI(i) = u() * (Y(ny - 1) - Y(0) + 0.6) + Y(0) - 0.3;
    arma::uword p = 0;
    for (arma::uword k : {0u, 2u, 4u, 6u, 9u, 11u, 14u, 17u, 21u, 22u}) {    // on, beside and midway: nine exact ties
        XI(p++) = X(k);
        XI(p++) = std::nextafter(X(k), -inf);
        XI(p++) = std::nextafter(X(k), inf);
        if (k + 1 < nx) XI(p++) = 0.5 * X(k) + 0.5 * X(k + 1);
    }
    XI(p++) = nan; XI(p++) = inf; XI(p++) = -inf;
    p = 0;
    for (arma::uword k : {0u, 1u, 3u, 4u, 7u, 8u, 10u, 12u, 15u, 16u}) {
        YI(p++) = Y(k);
        YI(p++) = std::nextafter(Y(k), -inf);
        YI(p++) = std::nextafter(Y(k), inf);
        if (k + 1 < ny) YI(p++) = 0.5 * Y(k) + 0.5 * Y(k + 1);
    }
    YI(p++) = nan; YI(p++) = inf; YI(p++) = -inf;

    arma::mat N, NE, L, LD, D, I0;
    mi355::interp2(X, Y, Z, XI, YI, N, "nearest");
    mi355::interp2(X, Y, Z, XI, YI, NE, "nearest", -7.5);
    mi355::interp2(X, Y, Z, XI, YI, L, "linear", 2.5);
    mi355::interp2(X, Y, Z, XI, YI, LD);                 // no seventh argument: the linear overload, extrap NaN
    mi355::interp2(X, Y, Z, XI, YI, D, 2.5);             // a double one: the linear overload, extrap 2.5
    mi355::interp2(X, Y, Z, XI, YI, I0, 0);              // an integer one: the linear overload too, extrap 0
    int threw_unknown = 0, threw_null = 0, threw_starred = 0;
    try { arma::mat W; mi355::interp2(X, Y, Z, XI, YI, W, "cubic"); } catch (const std::invalid_argument& e) {
        threw_unknown = std::string(e.what()) == "interp2(): unsupported interpolation type";
    }
    try { arma::mat W; mi355::interp2(X, Y, Z, XI, YI, W, "*nearest"); } catch (const std::invalid_argument&) { threw_starred = 1; }
    try { arma::mat W; mi355::interp2(X, Y, Z, XI, YI, W, (const char*)nullptr); } catch (const std::invalid_argument&) { threw_null = 1; }
    std::printf("threw_unknown %d\nthrew_starred %d\nthrew_null %d\n", threw_unknown, threw_starred, threw_null);
    std::printf("shape %llu %llu\n", (unsigned long long)N.n_rows, (unsigned long long)N.n_cols);
    dump(out + "/n2_X.bin", X);
    dump(out + "/n2_Y.bin", Y);
    dump(out + "/n2_Z.bin", Z);
    dump(out + "/n2_XI.bin", XI);
    dump(out + "/n2_YI.bin", YI);
    dump(out + "/n2_N.bin", N);
    dump(out + "/n2_NE.bin", NE);
    dump(out + "/n2_L.bin", L);
    dump(out + "/n2_LD.bin", LD);
    dump(out + "/n2_D.bin", D);
    dump(out + "/n2_I0.bin", I0);
    std::printf("arma_interp2_nearest_test done\n");
    return 0;
}
