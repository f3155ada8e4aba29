// GPU test of arma::interp2's gridded form in include/mi355_arma.hpp: mi355::interp2(X, Y, Z, XI, YI, arma::mat& ZI)
// and GroupInterp2Table::operator()(XI, YI, arma::mat&), next to the scattered arma::vec overload on the meshgrid pairs.
// Writes the inputs and results as raw doubles (and the result dimensions as text) so that the Python test can compare
// them with the oracle bit for bit.
//   arma_interp2_grid_test OUT_DIR
#include <cmath>
#include <cstdio>
#include <limits>
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
    const arma::uword nx = 37, ny = 23, nxi = 61, nyi = 45;
    arma::vec X(nx), Y(ny), XI(nxi), YI(nyi);
    arma::mat Z(ny, nx);
    for (arma::uword j = 0; j < nx; ++j) X(j) = 0.1 * j * (1.0 + 0.01 * j);           // non-uniform
    for (arma::uword i = 0; i < ny; ++i) Y(i) = -1.0 + 0.2 * i + 0.001 * i * i;
    for (arma::uword j = 0; j < nx; ++j)
        for (arma::uword i = 0; i < ny; ++i) Z(i, j) = std::sin(X(j)) * std::cos(Y(i)) + 0.1 * X(j) * Y(i);
    unsigned long long s = 7;
    auto u = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * 0x1.0p-53; };
    for (arma::uword j = 0; j < nxi; ++j) XI(j) = u() * (X(nx - 1) + 0.4) - 0.2;     // unsorted, some out of range
    for (arma::uword i = 0; i < nyi; ++i) YI(i) = u() * (Y(ny - 1) - Y(0) + 0.4) + Y(0) - 0.2;
    XI(3) = X(0); XI(4) = X(nx - 1); XI(5) = X(17); XI(6) = std::numeric_limits<double>::quiet_NaN();
    YI(2) = Y(ny - 1); YI(7) = Y(0); YI(8) = Y(11); YI(9) = std::numeric_limits<double>::quiet_NaN();

    arma::mat ZI;
    mi355::interp2(X, Y, Z, XI, YI, ZI);                       // arma::interp2's gridded form
    arma::mat ZE;
    mi355::interp2(X, Y, Z, XI, YI, ZE, -7.5);
    arma::vec PX(nxi * nyi), PY(nxi * nyi), ZS;                 // the meshgrid pairs, column-major
    for (arma::uword j = 0; j < nxi; ++j)
        for (arma::uword i = 0; i < nyi; ++i) { PX(i + j * nyi) = XI(j); PY(i + j * nyi) = YI(i); }
    mi355::interp2(X, Y, Z, PX, PY, ZS);                        // arma::vec: still the scattered overload
    arma::mat ZG;
    {
        mi355::DeviceGroup grp(std::vector<int>{0, 0, 0});     // GPU 0 named three times: three column shards
        mi355::GroupInterp2Table tab(grp, X, Y, Z);
        tab(XI, YI, ZG);
    }
    std::printf("ZI %llu %llu\nZE %llu %llu\nZS %llu %llu\nZG %llu %llu\n", (unsigned long long)ZI.n_rows,
                (unsigned long long)ZI.n_cols, (unsigned long long)ZE.n_rows, (unsigned long long)ZE.n_cols,
                (unsigned long long)ZS.n_rows, (unsigned long long)ZS.n_cols, (unsigned long long)ZG.n_rows,
                (unsigned long long)ZG.n_cols);
    dump(out + "/g_X.bin", X.memptr(), X.n_elem);
    dump(out + "/g_Y.bin", Y.memptr(), Y.n_elem);
    dump(out + "/g_Z.bin", Z.memptr(), Z.n_elem);
    dump(out + "/g_XI.bin", XI.memptr(), XI.n_elem);
    dump(out + "/g_YI.bin", YI.memptr(), YI.n_elem);
    dump(out + "/g_ZI.bin", ZI.memptr(), ZI.n_elem);
    dump(out + "/g_ZE.bin", ZE.memptr(), ZE.n_elem);
    dump(out + "/g_ZS.bin", ZS.memptr(), ZS.n_elem);
    dump(out + "/g_ZG.bin", ZG.memptr(), ZG.n_elem);
    std::printf("arma_interp2_grid_test done\n");
    return 0;
}
