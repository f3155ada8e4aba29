// GPU test of arma::interp1's method strings in include/mi355_arma.hpp: mi355::interp1(X, Y, XI, YI, method, extrap) with
// "linear", "*linear", "nearest", "*nearest" and an unknown string (which must throw std::invalid_argument), a double
// (and an integer) fifth argument still reaching the linear overload, and Interp1Table::nearest.  Writes the inputs and
// results as raw doubles so that the Python test can compare them with its numpy references bit for bit.
//   arma_interp1_nearest_test OUT_DIR
#include <cmath>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <string>

#include "mi355_arma.hpp"

static void dump(const std::string& path, const arma::vec& v)
{
    FILE* fp = std::fopen(path.c_str(), "wb");
    std::fwrite(v.memptr(), sizeof(double), v.n_elem, fp);
    std::fclose(fp);
}

int main(int argc, char** argv)
{
    const std::string out = argc > 1 ? argv[1] : ".";
    const arma::uword n = 401, nxi = 1203;
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    arma::vec X(n), Y(n), XP(n), YP(n), XI(nxi);
    for (arma::uword i = 0; i < n; ++i) {
        X(i) = -1.0 + 0.03 * i * (1.0 + 0.001 * i);                          // non-uniform, strictly increasing
        Y(i) = std::sin(3.0 * X(i)) + 0.125 * i;
    }
    Y(5) = inf; Y(6) = -inf; Y(17) = nan; Y(40) = -0.0; Y(41) = -0.0; Y(n - 1) = nan; Y(0) = -0.0;
    for (arma::uword i = 0; i < n; ++i) {                                    // a permutation of the table (173 is coprime to 401)
        const arma::uword j = (i * 173u + 7u) % n;
        XP(i) = X(j);
        YP(i) = Y(j);
    }
    unsigned long long s = 29;
    auto u = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * 0x1.0p-53; };
    for (arma::uword j = 0; j < nxi; ++j) XI(j) = u() * (X(n - 1) - X(0) + 0.6) + X(0) - 0.3;   // unsorted, some out of range
    arma::uword p = 0;
    for (arma::uword k : {0u, 4u, 5u, 6u, 16u, 17u, 18u, 40u, 41u, 399u, 400u}) {             // on, beside and midway
        XI(p++) = X(k);
        XI(p++) = std::nextafter(X(k), -inf);
        XI(p++) = std::nextafter(X(k), inf);
        if (k + 1 < n) XI(p++) = 0.5 * X(k) + 0.5 * X(k + 1);
    }
    XI(p++) = nan; XI(p++) = inf; XI(p++) = -inf;

    arma::vec L, SL, N, SN, NE, D, I0, T, TL;
    mi355::interp1(X, Y, XI, D, 2.5);                   // a double fifth argument: the linear overload, extrap 2.5
    mi355::interp1(X, Y, XI, I0, 0);                    // an integer one: the linear overload too, extrap 0
    mi355::interp1(XP, YP, XI, L, "linear", 2.5);       // sanitising: the permuted table
    mi355::interp1(X, Y, XI, SL, "*linear", 2.5);
    mi355::interp1(XP, YP, XI, N, "nearest");
    mi355::interp1(X, Y, XI, SN, "*nearest");
    mi355::interp1(XP, YP, XI, NE, "nearest", -7.5);
    mi355::Interp1Table tab(X, Y, false);
    tab.nearest(XI, T, -7.5);
    tab(XI, TL, 2.5);
    int threw_unknown = 0, threw_unsorted = 0, threw_null = 0;
    try { arma::vec Z; mi355::interp1(X, Y, XI, Z, "cubic"); } catch (const std::invalid_argument& e) {
        threw_unknown = std::string(e.what()) == "interp1(): unsupported interpolation type";
    }
    try { arma::vec Z; mi355::interp1(X, Y, XI, Z, (const char*)nullptr); } catch (const std::invalid_argument&) { threw_null = 1; }
    try { arma::vec Z; mi355::interp1(XP, YP, XI, Z, "*nearest"); } catch (const std::runtime_error&) { threw_unsorted = 1; }
    std::printf("threw_unknown %d\nthrew_null %d\nthrew_unsorted %d\n", threw_unknown, threw_null, threw_unsorted);
    dump(out + "/n_X.bin", X);
    dump(out + "/n_Y.bin", Y);
    dump(out + "/n_XI.bin", XI);
    dump(out + "/n_D.bin", D);
    dump(out + "/n_I0.bin", I0);
    dump(out + "/n_L.bin", L);
    dump(out + "/n_SL.bin", SL);
    dump(out + "/n_N.bin", N);
    dump(out + "/n_SN.bin", SN);
    dump(out + "/n_NE.bin", NE);
    dump(out + "/n_T.bin", T);
    dump(out + "/n_TL.bin", TL);
    std::printf("arma_interp1_nearest_test done\n");
    return 0;
}
