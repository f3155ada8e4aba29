// GPU test of interp1 over paired columns with a query vector per column in include/mi355_arma.hpp: mi355::interp1_each
// and GroupInterp1Each, on a table long enough for the LDS form and on two-node columns with one query each (the thin
// kernel).  Writes the inputs and results as raw doubles (and the result dimensions as text) so that the Python test can
// compare them with the oracle bit for bit.
//   arma_interp1_each_test OUT_DIR
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "mi355_arma.hpp"

static void dump(const std::string& path, const void* p, size_t bytes)
{
    FILE* fp = std::fopen(path.c_str(), "wb");
    std::fwrite(p, 1, bytes, fp);
    std::fclose(fp);
}

static void dump(const std::string& path, const arma::mat& m) { dump(path, m.memptr(), m.n_elem * sizeof(double)); }

int main(int argc, char** argv)
{
    const std::string out = argc > 1 ? argv[1] : ".";
    const double nan = std::numeric_limits<double>::quiet_NaN();
    unsigned long long s = 17;
    auto u = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * 0x1.0p-53; };

    // long columns: every column has its own range, and its queries are drawn around that range
    const arma::uword n = 301, B = 29, nxi = 157;
    arma::mat X(n, B), Y(n, B), XI(nxi, B);
    for (arma::uword c = 0; c < B; ++c) {
        for (arma::uword i = 0; i < n; ++i) {
            X(i, c) = -2.0 + 30.0 * c + 0.05 * i * (1.0 + 0.002 * i + 0.01 * c);
            Y(i, c) = std::sin(X(i, c) * (1.0 + 0.1 * c)) + 0.01 * c * X(i, c);
        }
        const double lo = X(0, c), hi = X(n - 1, c);
        for (arma::uword j = 0; j < nxi; ++j) XI(j, c) = u() * (hi - lo + 0.4) + lo - 0.2;   // unsorted, some out of range
        XI(3, c) = lo; XI(4, c) = hi; XI(5, c) = X(7, c); XI(6, c) = nan; XI(7, c) = X(9, c);
    }
    Y(7, 3) = std::numeric_limits<double>::infinity();
    Y(8, 4) = nan;
    Y(9, 5) = -0.0;
    X(100, 11) = X(99, 11);                                  // equal neighbours: column 11 is bad
    X(n - 1, 20) = nan;                                      // column 20 too

    arma::mat YP, YE, YG, YT;
    std::vector<uint32_t> ok, oke, okg;
    mi355::interp1_each(X, Y, XI, YP, nan, mi355::Device::instance(), &ok);
    mi355::interp1_each(X, Y, XI, YE, -7.5, mi355::Device::instance(), &oke);
    {
        mi355::DeviceGroup grp(std::vector<int>{0, 0, 0});   // GPU 0 named three times: three column shards
        mi355::GroupInterp1Each ge(grp);
        ge(X, Y, XI, YG, nan, &okg);
    }

    // two-node columns, one query each: Restrict with a horizon per realisation
    const arma::uword B2 = 1000;
    arma::mat X2(2, B2), Y2(2, B2), Q2(1, B2), YR, YRG;
    for (arma::uword c = 0; c < B2; ++c) {
        X2(0, c) = 10.0 * c + u();
        X2(1, c) = X2(0, c) + 0.5 + u();
        Y2(0, c) = u() - 0.5;
        Y2(1, c) = u() + 3.0;
        Q2(0, c) = X2(0, c) + 1.7 * u() - 0.1;               // mostly inside, some outside on either side
    }
    Q2(0, 1) = X2(0, 1); Q2(0, 2) = X2(1, 2); Q2(0, 3) = nan;
    X2(1, 500) = X2(0, 500);                                 // bad
    std::vector<uint32_t> ok2, ok2g;
    mi355::interp1_each(X2, Y2, Q2, YR, 99.0, mi355::Device::instance(), &ok2);
    {
        mi355::DeviceGroup grp(std::vector<int>{0, 0, 0});
        mi355::GroupInterp1Each ge(grp);
        ge(X2, Y2, Q2, YRG, 99.0, &ok2g);
    }

    // without an ok vector a bad column is an error (MI_ERR_GRID), reported after YI is complete
    int threw_bad = 0;
    try {
        mi355::interp1_each(X, Y, XI, YT);
    } catch (const std::runtime_error&) {
        threw_bad = 1;
    }
    arma::mat YC(nxi, B);
    const mi_status bad_status = mi_interp1_each_f64_host(mi355::Device::instance().get(), X.memptr(), n, Y.memptr(), n, n, nullptr, B,
                                                          XI.memptr(), nxi, nxi, YC.memptr(), nxi, nan, nullptr);
    int threw = 0;
    try {
        arma::mat Ybad(n - 1, B), T;
        mi355::interp1_each(X, Ybad, XI, T);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    try {
        arma::mat XIbad(nxi, B - 1), T;
        mi355::interp1_each(X, Y, XIbad, T);
    } catch (const std::invalid_argument&) {
        ++threw;
    }
    std::printf("YP %llu %llu\nYE %llu %llu\nYG %llu %llu\nYR %llu %llu\nYRG %llu %llu\nthrew %d\nthrew_bad %d\nbad_status %d\n",
                (unsigned long long)YP.n_rows, (unsigned long long)YP.n_cols, (unsigned long long)YE.n_rows,
                (unsigned long long)YE.n_cols, (unsigned long long)YG.n_rows, (unsigned long long)YG.n_cols,
                (unsigned long long)YR.n_rows, (unsigned long long)YR.n_cols, (unsigned long long)YRG.n_rows,
                (unsigned long long)YRG.n_cols, threw, threw_bad, (int)bad_status);
    const uint32_t n32 = (uint32_t)n;
    dump(out + "/e_N.bin", &n32, sizeof(n32));
    dump(out + "/e_X.bin", X);
    dump(out + "/e_Y.bin", Y);
    dump(out + "/e_XI.bin", XI);
    dump(out + "/e_YP.bin", YP);
    dump(out + "/e_YE.bin", YE);
    dump(out + "/e_YG.bin", YG);
    dump(out + "/e_X2.bin", X2);
    dump(out + "/e_Y2.bin", Y2);
    dump(out + "/e_Q2.bin", Q2);
    dump(out + "/e_YR.bin", YR);
    dump(out + "/e_YRG.bin", YRG);
    dump(out + "/e_OK.bin", ok.data(), ok.size() * sizeof(uint32_t));
    dump(out + "/e_OKG.bin", okg.data(), okg.size() * sizeof(uint32_t));
    dump(out + "/e_OK2.bin", ok2.data(), ok2.size() * sizeof(uint32_t));
    dump(out + "/e_OK2G.bin", ok2g.data(), ok2g.size() * sizeof(uint32_t));
    if (!threw_bad || ok != oke) return 1;
    std::printf("arma_interp1_each_test done\n");
    return 0;
}
