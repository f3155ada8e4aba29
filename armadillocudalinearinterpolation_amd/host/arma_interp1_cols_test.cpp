// GPU test of interp1 over the columns of a matrix in include/mi355_arma.hpp: mi355::Interp1Axis, the one-shot
// mi355::interp1(X, arma::mat Y, XI, arma::mat& YI) and GroupInterp1Axis, next to the arma::vec overload (Interp1Table
// without sanitising) column by column.  Writes the inputs and results as raw doubles (and the result dimensions as text)
// so that the Python test can compare them with the oracle bit for bit.
//   arma_interp1_cols_test OUT_DIR
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "mi355_arma.hpp"

static void dump(const std::string& path, const double* p, size_t n)
{
    FILE* fp = std::fopen(path.c_str(), "wb");
    std::fwrite(p, sizeof(double), n, fp);
    std::fclose(fp);
}

int main(int argc, char** argv)
{
    const std::string out = argc > 1 ? argv[1] : ".";
    const arma::uword n = 301, B = 29, nxi = 157;
    arma::vec X(n), XI(nxi);
    arma::mat Y(n, B);
    for (arma::uword i = 0; i < n; ++i) X(i) = -2.0 + 0.05 * i * (1.0 + 0.002 * i);          // non-uniform
    for (arma::uword c = 0; c < B; ++c)
        for (arma::uword i = 0; i < n; ++i) Y(i, c) = std::sin(X(i) * (1.0 + 0.1 * c)) + 0.01 * c * X(i);
    Y(7, 3) = std::numeric_limits<double>::infinity();
    Y(8, 4) = std::numeric_limits<double>::quiet_NaN();
    Y(9, 5) = -0.0;
    unsigned long long s = 11;
    auto u = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * 0x1.0p-53; };
    for (arma::uword j = 0; j < nxi; ++j) XI(j) = u() * (X(n - 1) - X(0) + 0.4) + X(0) - 0.2;   // unsorted, some out of range
    XI(3) = X(0); XI(4) = X(n - 1); XI(5) = X(7); XI(6) = std::numeric_limits<double>::quiet_NaN(); XI(7) = X(9);

    arma::mat YA, YE, YO, YG, YV(nxi, B);
    mi355::Interp1Axis axis(X);
    axis(Y, XI, YA);                                    // the resident axis
    axis(Y, XI, YE, -7.5);
    mi355::interp1(X, Y, XI, YO);                       // one-shot, matrices
    for (arma::uword c = 0; c < B; ++c) {               // arma::vec: still the per-table overload
        arma::vec yc(n), yi;
        for (arma::uword i = 0; i < n; ++i) yc(i) = Y(i, c);
        mi355::Interp1Table tab(X, yc, false);
        tab(XI, yi);
        for (arma::uword j = 0; j < nxi; ++j) YV(j, c) = yi(j);
    }
    {
        mi355::DeviceGroup grp(std::vector<int>{0, 0, 0});   // GPU 0 named three times: three column shards
        mi355::GroupInterp1Axis gax(grp, X);
        gax(Y, XI, YG);
    }
    int threw = 0;
    try {
        arma::mat Ybad(n - 1, B), T;
        axis(Ybad, XI, T);
    } catch (const std::invalid_argument&) {
        threw = 1;
    }
    std::printf("YA %llu %llu\nYE %llu %llu\nYO %llu %llu\nYG %llu %llu\nthrew %d\n", (unsigned long long)YA.n_rows,
                (unsigned long long)YA.n_cols, (unsigned long long)YE.n_rows, (unsigned long long)YE.n_cols,
                (unsigned long long)YO.n_rows, (unsigned long long)YO.n_cols, (unsigned long long)YG.n_rows,
                (unsigned long long)YG.n_cols, threw);
    dump(out + "/c_X.bin", X.memptr(), X.n_elem);
    dump(out + "/c_Y.bin", Y.memptr(), Y.n_elem);
    dump(out + "/c_XI.bin", XI.memptr(), XI.n_elem);
    dump(out + "/c_YA.bin", YA.memptr(), YA.n_elem);
    dump(out + "/c_YE.bin", YE.memptr(), YE.n_elem);
    dump(out + "/c_YO.bin", YO.memptr(), YO.n_elem);
    dump(out + "/c_YV.bin", YV.memptr(), YV.n_elem);
    dump(out + "/c_YG.bin", YG.memptr(), YG.n_elem);
    std::printf("arma_interp1_cols_test done\n");
    return 0;
}
