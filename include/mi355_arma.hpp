// mi355_arma.hpp -- Armadillo-facing C++ operator signatures over the C ABI
// (include/mi355_interp.h): arma::vec / arma::mat in, interpolated arma::vec
// out, as BASELINE.json's north_star asks.  Header-only; link libmi355interp.so.
//
//   mi355::interp1(X, Y, XI, YI)            == arma::interp1(X, Y, XI, YI, "linear")
//   mi355::interp1(X, Y, XI, YI, method)    == arma::interp1(X, Y, XI, YI, method): "linear", "*linear", "nearest",
//                                           "*nearest" (the starred forms take X as given: strictly increasing, else throw)
//   mi355::Interp1Table tab(X, Y); tab(XI, YI)   table resident in HBM across calls
//                       tab.nearest(XI, YI)      the "nearest" method on the same resident table
//   mi355::interp1(X, Y, XI, YI)            Y, YI arma::mat: interp1 on every column of Y (MATLAB's interp1 with a matrix
//                                           Y), YI = XI.n_elem x Y.n_cols; X as given ("*linear": strictly increasing)
//   mi355::Interp1Axis ax(X); ax(Y, XI, YI)      the axis resident across calls while Y changes
//   mi355::interp1_paired(X, Y, XI, YI)     X, Y, YI arma::mat: column c of Y sampled at the nodes in column c of X (an X
//                                           per column: an ensemble of trajectories onto one mesh), YI = XI.n_elem x
//                                           Y.n_cols; a column whose X is not finite and strictly increasing is all NaN
//   mi355::GroupInterp1Paired gp(grp); gp(X, Y, XI, YI)   the same with the columns sharded over the GPUs of the node
//   mi355::interp1_each(X, Y, XI, YI)       X, Y, XI, YI arma::mat: as interp1_paired with a query vector per column, column c
//                                           of XI for column c of (X, Y); YI = XI.n_rows x Y.n_cols.  Very short columns
//                                           (two-node Restrict-like tables) take a thin one-lane-per-column kernel
//   mi355::GroupInterp1Each ge(grp); ge(X, Y, XI, YI)      the same with the columns (and XI's) sharded over the GPUs
//   mi355::interp2(X, Y, Z, XI, YI, ZI)     ZI an arma::mat: == arma::interp2(X, Y, Z, XI, YI, ZI, "linear", extrap),
//                                           ZI = YI.n_elem x XI.n_elem; Z = arma::mat(Y.n_elem, X.n_elem)
//                                           ZI an arma::vec: scattered extension, one result per (XI[k], YI[k]) pair
//   mi355::interp2(X, Y, Z, XI, YI, ZI, method)   ZI an arma::mat: == arma::interp2(..., method, extrap): "linear" or
//                                           "nearest" (ZI(i, j) = Z(ky, kx), the stored value of the nearest node on each
//                                           axis, a tie keeps the left node); any other string throws
//   mi355::restrict_to_horizon(...)         RestrictKernel (EventDrivenMap.cu:769-785) on host vectors
//   mi355::DeviceGroup grp(8); mi355::GroupInterp1Table tab(grp, X, Y); tab(XI, YI)
//                                           the same call with the queries sharded over the GPUs of the node
//
// Error convention: the reference aborts on any device error (CUDA_CALL ->
// fprintf(stderr) + exit(-1), EventDrivenMap.cu:18-54) and on bad arguments
// (assert); Armadillo itself throws.  These wrappers throw std::runtime_error
// carrying mi_last_error(); mi355::abort_on_error(true) restores print + exit(-1).
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <stdexcept>
#include <cstdint>
#include <string>
#include <type_traits>
#include <vector>

#include "mi355_arma_compat.hpp"
#include "mi355_interp.h"

namespace mi355 {

inline bool& abort_flag() { static bool f = false; return f; }
inline void abort_on_error(bool on) { abort_flag() = on; }

inline void check(mi_status st, const mi_ctx* ctx, const char* where)
{
    if (st == MI_OK) return;
    std::string msg = std::string(where) + ": " + mi_last_error(ctx);
    if (abort_flag()) {
        std::fprintf(stderr, "%s\n", msg.c_str());
        std::exit(-1);
    }
    throw std::runtime_error(msg);
}

// One context per device, created on first use.
class Device {
  public:
    explicit Device(int ordinal = 0) : ctx_(nullptr) { check(mi_ctx_create(ordinal, &ctx_), nullptr, "mi_ctx_create"); }
    ~Device() { mi_ctx_destroy(ctx_); }
    Device(const Device&) = delete;
    Device& operator=(const Device&) = delete;
    mi_ctx* get() const { return ctx_; }
    static Device& instance()
    {
        static Device d(0);
        return d;
    }

  private:
    mi_ctx* ctx_;
};

// A 1-D table kept in HBM: build once, interpolate many query vectors.
class Interp1Table {
  public:
    // sanitise = true reproduces arma::interp1's default (X sorted and de-duplicated first);
    // false is its "*linear" fast path (X must already be strictly increasing).
    Interp1Table(const arma::vec& X, const arma::vec& Y, bool sanitise = true, Device& dev = Device::instance())
        : dev_(dev), g_(nullptr)
    {
        if (X.n_elem != Y.n_elem) throw std::invalid_argument("interp1(): X and Y must have the same number of elements");
        check(mi_grid1_create(dev_.get(), X.memptr(), Y.memptr(), X.n_elem, sanitise ? MI_GRID_SANITISE : 0u, &g_),
              dev_.get(), "mi_grid1_create");
    }
    ~Interp1Table() { mi_grid1_destroy(g_); }
    Interp1Table(const Interp1Table&) = delete;
    Interp1Table& operator=(const Interp1Table&) = delete;

    void operator()(const arma::vec& XI, arma::vec& YI, double extrap_val = std::numeric_limits<double>::quiet_NaN()) const
    {
        YI.set_size(XI.n_elem);
        check(mi_interp1_f64_host(dev_.get(), g_, XI.memptr(), YI.memptr(), XI.n_elem, extrap_val), dev_.get(),
              "mi_interp1_f64_host");
    }

    // arma::interp1's "nearest" method on the same resident table: YI[i] = Y[k], k the node nearest to XI[i]
    // (a tie keeps the left node; the stored value comes back as it is)
    void nearest(const arma::vec& XI, arma::vec& YI, double extrap_val = std::numeric_limits<double>::quiet_NaN()) const
    {
        YI.set_size(XI.n_elem);
        check(mi_interp1_nearest_f64_host(dev_.get(), g_, XI.memptr(), YI.memptr(), XI.n_elem, extrap_val), dev_.get(),
              "mi_interp1_nearest_f64_host");
    }

  private:
    Device& dev_;
    mi_grid1* g_;
};

// arma::interp1(X, Y, XI, YI, "linear", extrap_val)
inline void interp1(const arma::vec& X, const arma::vec& Y, const arma::vec& XI, arma::vec& YI,
                    double extrap_val = std::numeric_limits<double>::quiet_NaN(), Device& dev = Device::instance())
{
    if (X.n_elem != Y.n_elem) throw std::invalid_argument("interp1(): X and Y must have the same number of elements");
    YI.set_size(XI.n_elem);
    check(mi_interp1_f64(dev.get(), X.memptr(), Y.memptr(), X.n_elem, XI.memptr(), YI.memptr(), XI.n_elem, extrap_val),
          dev.get(), "mi_interp1_f64");
}

// arma::interp1(X, Y, XI, YI, method, extrap_val) with Armadillo's four method strings:
//   "linear"    X sorted and de-duplicated first, the fp64 blend             (mi_interp1_f64, as the overload above)
//   "*linear"   X used as given, must be strictly increasing (else throws)   (mi_interp1_f64_host)
//   "nearest"   X sorted and de-duplicated first, the nearest rule           (mi_interp1_nearest_f64)
//   "*nearest"  X used as given, must be strictly increasing (else throws)   (mi_interp1_nearest_f64_host)
// anything else throws std::invalid_argument, as Armadillo does.
inline void interp1(const arma::vec& X, const arma::vec& Y, const arma::vec& XI, arma::vec& YI, const char* method,
                    double extrap_val = std::numeric_limits<double>::quiet_NaN(), Device& dev = Device::instance())
{
    const std::string m = method ? method : "";
    if (m == "linear") return interp1(X, Y, XI, YI, extrap_val, dev);
    if (m == "*linear") return Interp1Table(X, Y, false, dev)(XI, YI, extrap_val);
    if (m == "*nearest") return Interp1Table(X, Y, false, dev).nearest(XI, YI, extrap_val);
    if (m != "nearest") throw std::invalid_argument("interp1(): unsupported interpolation type");
    if (X.n_elem != Y.n_elem) throw std::invalid_argument("interp1(): X and Y must have the same number of elements");
    YI.set_size(XI.n_elem);
    check(mi_interp1_nearest_f64(dev.get(), X.memptr(), Y.memptr(), X.n_elem, XI.memptr(), YI.memptr(), XI.n_elem, extrap_val),
          dev.get(), "mi_interp1_nearest_f64");
}

// an integer extrapolation value (a literal 0 among them) still means the linear overload: without this the null
// pointer conversion to `const char* method` would compete with the conversion to double
template <typename T, typename std::enable_if<std::is_integral<T>::value, int>::type = 0>
inline void interp1(const arma::vec& X, const arma::vec& Y, const arma::vec& XI, arma::vec& YI, T extrap_val,
                    Device& dev = Device::instance())
{
    interp1(X, Y, XI, YI, (double)extrap_val, dev);
}

// interp1 over the columns of a matrix: YI(:, c) = arma::interp1(X, Y.col(c), XI, YI.col(c), "*linear", extrap_val) for
// every column c, bit-identical to Interp1Table(X, Y.col(c), false) on XI.  The axis is validated and uploaded once and
// reused while Y changes.  "*linear" contract: X is used as given and must be strictly increasing and finite (it is not
// sorted or de-duplicated for the caller, which would mean permuting the rows of every Y); otherwise the call throws.
class Interp1Axis {
  public:
    explicit Interp1Axis(const arma::vec& X, Device& dev = Device::instance()) : dev_(dev), a_(nullptr), n_(X.n_elem)
    {
        check(mi_axis1_create(dev_.get(), X.memptr(), X.n_elem, 0u, &a_), dev_.get(), "mi_axis1_create");
    }
    // nodes fma(i, dx, x0), i < n
    Interp1Axis(double x0, double dx, size_t n, Device& dev = Device::instance()) : dev_(dev), a_(nullptr), n_(n)
    {
        check(mi_axis1_create_uniform(dev_.get(), x0, dx, n, &a_), dev_.get(), "mi_axis1_create_uniform");
    }
    ~Interp1Axis() { mi_axis1_destroy(a_); }
    Interp1Axis(const Interp1Axis&) = delete;
    Interp1Axis& operator=(const Interp1Axis&) = delete;

    void operator()(const arma::mat& Y, const arma::vec& XI, arma::mat& YI,
                    double extrap_val = std::numeric_limits<double>::quiet_NaN()) const
    {
        if (Y.n_rows != n_) throw std::invalid_argument("interp1(): Y must have X.n_elem rows");
        YI.set_size(XI.n_elem, Y.n_cols);
        check(mi_interp1_cols_f64_host(dev_.get(), a_, Y.memptr(), Y.n_rows, Y.n_cols, XI.memptr(), XI.n_elem, YI.memptr(),
                                       XI.n_elem, extrap_val),
              dev_.get(), "mi_interp1_cols_f64_host");
    }

  private:
    Device& dev_;
    mi_axis1* a_;
    size_t n_;
};

// one-shot form: Y, YI matrices (the vector overload above is arma::interp1 itself)
inline void interp1(const arma::vec& X, const arma::mat& Y, const arma::vec& XI, arma::mat& YI,
                    double extrap_val = std::numeric_limits<double>::quiet_NaN(), Device& dev = Device::instance())
{
    if (Y.n_rows != X.n_elem) throw std::invalid_argument("interp1(): Y must have X.n_elem rows");
    Interp1Axis(X, dev)(Y, XI, YI, extrap_val);
}

// interp1 over paired columns: YI(:, c) = arma::interp1(X.col(c), Y.col(c), XI, YI.col(c), "*linear", extrap_val) for
// every column c, bit-identical to Interp1Table(X.col(c), Y.col(c), false) on XI.  A name of its own: an arma::mat X
// overload of interp1 would compete with the arma::vec one wherever Col derives from Mat.  Every column of X is validated
// on the device ("*linear" contract: used as given, finite and strictly increasing); a column that is not comes back
// all NaN.  With ok == nullptr such a column also makes the call throw (YI is complete all the same); with an ok vector
// the call reports ok[c] = 1 / 0 instead and does not throw for it.
inline void interp1_paired(const arma::mat& X, const arma::mat& Y, const arma::vec& XI, arma::mat& YI,
                           double extrap_val = std::numeric_limits<double>::quiet_NaN(), Device& dev = Device::instance(),
                           std::vector<uint32_t>* ok = nullptr)
{
    if (X.n_rows != Y.n_rows || X.n_cols != Y.n_cols) throw std::invalid_argument("interp1_paired(): X and Y must have the same shape");
    YI.set_size(XI.n_elem, Y.n_cols);
    if (ok) ok->assign(Y.n_cols, 1u);
    check(mi_interp1_pairs_f64_host(dev.get(), X.memptr(), X.n_rows, Y.memptr(), Y.n_rows, X.n_rows, nullptr, Y.n_cols,
                                    XI.memptr(), XI.n_elem, YI.memptr(), XI.n_elem, extrap_val, ok ? ok->data() : nullptr),
          dev.get(), "mi_interp1_pairs_f64_host");
}

// interp1 over paired columns with a query vector per column: YI(:, c) = arma::interp1(X.col(c), Y.col(c), XI.col(c),
// YI.col(c), "*linear", extrap_val) for every column c.  Validation, NaN columns, ok and the throwing rule are
// interp1_paired's; XI must have as many columns as X.
inline void interp1_each(const arma::mat& X, const arma::mat& Y, const arma::mat& XI, arma::mat& YI,
                         double extrap_val = std::numeric_limits<double>::quiet_NaN(), Device& dev = Device::instance(),
                         std::vector<uint32_t>* ok = nullptr)
{
    if (X.n_rows != Y.n_rows || X.n_cols != Y.n_cols) throw std::invalid_argument("interp1_each(): X and Y must have the same shape");
    if (XI.n_cols != X.n_cols) throw std::invalid_argument("interp1_each(): XI must have as many columns as X");
    YI.set_size(XI.n_rows, Y.n_cols);
    if (ok) ok->assign(Y.n_cols, 1u);
    check(mi_interp1_each_f64_host(dev.get(), X.memptr(), X.n_rows, Y.memptr(), Y.n_rows, X.n_rows, nullptr, Y.n_cols,
                                   XI.memptr(), XI.n_rows, XI.n_rows, YI.memptr(), XI.n_rows, extrap_val,
                                   ok ? ok->data() : nullptr),
          dev.get(), "mi_interp1_each_f64_host");
}

// Scattered bilinear interpolation (an extension, not an Armadillo call): ZI[k] = Z(YI[k], XI[k]); Z is
// Y.n_elem x X.n_elem (rows follow Y), the layout arma::interp2 uses for its Z argument.  One result per query PAIR.
// With the real Armadillo an arma::vec ZI binds here (exact match) rather than to the arma::mat overload below.
inline void interp2(const arma::vec& X, const arma::vec& Y, const arma::mat& Z, const arma::vec& XI,
                    const arma::vec& YI, arma::vec& ZI,
                    double extrap_val = std::numeric_limits<double>::quiet_NaN(), Device& dev = Device::instance())
{
    if (Z.n_rows != Y.n_elem || Z.n_cols != X.n_elem) throw std::invalid_argument("interp2(): Z must be Y.n_elem x X.n_elem");
    if (XI.n_elem != YI.n_elem) throw std::invalid_argument("interp2(): XI and YI must have the same number of elements");
    mi_grid2* g = nullptr;
    check(mi_grid2_create(dev.get(), X.memptr(), X.n_elem, Y.memptr(), Y.n_elem, Z.memptr(), 0u, &g), dev.get(),
          "mi_grid2_create");
    ZI.set_size(XI.n_elem);
    mi_status st = mi_interp2_f64_host(dev.get(), g, XI.memptr(), YI.memptr(), ZI.memptr(), XI.n_elem, extrap_val);
    mi_grid2_destroy(g);
    check(st, dev.get(), "mi_interp2_f64_host");
}

// arma::interp2(X, Y, Z, XI, YI, ZI, "linear", extrap_val): ZI = YI.n_elem x XI.n_elem, ZI(i, j) = Z at (XI[j], YI[i]),
// bit-identical to the scattered overload on that pair.
inline void interp2(const arma::vec& X, const arma::vec& Y, const arma::mat& Z, const arma::vec& XI,
                    const arma::vec& YI, arma::mat& ZI,
                    double extrap_val = std::numeric_limits<double>::quiet_NaN(), Device& dev = Device::instance())
{
    if (Z.n_rows != Y.n_elem || Z.n_cols != X.n_elem) throw std::invalid_argument("interp2(): Z must be Y.n_elem x X.n_elem");
    mi_grid2* g = nullptr;
    check(mi_grid2_create(dev.get(), X.memptr(), X.n_elem, Y.memptr(), Y.n_elem, Z.memptr(), 0u, &g), dev.get(),
          "mi_grid2_create");
    ZI.set_size(YI.n_elem, XI.n_elem);
    mi_status st = mi_interp2_grid_f64_host(dev.get(), g, XI.memptr(), XI.n_elem, YI.memptr(), YI.n_elem, ZI.memptr(),
                                            extrap_val);
    mi_grid2_destroy(g);
    check(st, dev.get(), "mi_interp2_grid_f64_host");
}

// arma::interp2(X, Y, Z, XI, YI, ZI, method, extrap_val) with Armadillo's two method strings (interp2 has no starred forms):
//   "linear"    the overload above                                                (mi_interp2_grid_f64_host)
//   "nearest"   ZI(i, j) = Z(ky, kx), the stored value of the node the nearest rule picks on each axis: a tie keeps the
//               left node, inf / NaN / -0.0 come back as they are             (mi_interp2_grid_nearest_f64_host)
// anything else throws std::invalid_argument, as Armadillo does.  XI and YI may be in any order.
inline void interp2(const arma::vec& X, const arma::vec& Y, const arma::mat& Z, const arma::vec& XI,
                    const arma::vec& YI, arma::mat& ZI, const char* method,
                    double extrap_val = std::numeric_limits<double>::quiet_NaN(), Device& dev = Device::instance())
{
    const std::string m = method ? method : "";
    if (m == "linear") return interp2(X, Y, Z, XI, YI, ZI, extrap_val, dev);
    if (m != "nearest") throw std::invalid_argument("interp2(): unsupported interpolation type");
    if (Z.n_rows != Y.n_elem || Z.n_cols != X.n_elem) throw std::invalid_argument("interp2(): Z must be Y.n_elem x X.n_elem");
    mi_grid2* g = nullptr;
    check(mi_grid2_create(dev.get(), X.memptr(), X.n_elem, Y.memptr(), Y.n_elem, Z.memptr(), 0u, &g), dev.get(),
          "mi_grid2_create");
    ZI.set_size(YI.n_elem, XI.n_elem);
    mi_status st = mi_interp2_grid_nearest_f64_host(dev.get(), g, XI.memptr(), XI.n_elem, YI.memptr(), YI.n_elem, ZI.memptr(),
                                                    extrap_val);
    mi_grid2_destroy(g);
    check(st, dev.get(), "mi_interp2_grid_nearest_f64_host");
}

// an integer extrapolation value (a literal 0 among them) still means the linear overloads: without these the null
// pointer conversion to `const char* method` would compete with the conversion to double.  One per kind of ZI: where
// arma::vec derives from arma::mat, a guard for arma::mat alone would tie with the scattered overload on an arma::vec ZI.
template <typename T, typename std::enable_if<std::is_integral<T>::value, int>::type = 0>
inline void interp2(const arma::vec& X, const arma::vec& Y, const arma::mat& Z, const arma::vec& XI, const arma::vec& YI,
                    arma::mat& ZI, T extrap_val, Device& dev = Device::instance())
{
    interp2(X, Y, Z, XI, YI, ZI, (double)extrap_val, dev);
}

template <typename T, typename std::enable_if<std::is_integral<T>::value, int>::type = 0>
inline void interp2(const arma::vec& X, const arma::vec& Y, const arma::mat& Z, const arma::vec& XI, const arma::vec& YI,
                    arma::vec& ZI, T extrap_val, Device& dev = Device::instance())
{
    interp2(X, Y, Z, XI, YI, ZI, (double)extrap_val, dev);
}

// RestrictKernel (EventDrivenMap.cu:769-785) on host vectors: position at t = final_time from the last event
// before (t0, i0) and the first event after (t1, i1) the horizon, on the implicit grid x_i = -L + 2L/N * i.
inline void restrict_to_horizon(const arma::fvec& t0, const std::vector<uint16_t>& i0, const arma::fvec& t1,
                                const std::vector<uint16_t>& i1, float final_time, float half_length,
                                unsigned int n_grid, arma::fvec& out, Device& dev = Device::instance())
{
    const size_t n = t0.n_elem;
    if (t1.n_elem != n || i0.size() != n || i1.size() != n) throw std::invalid_argument("restrict_to_horizon(): size mismatch");
    out.set_size(n);
    check(mi_restrict_f32_host(dev.get(), t0.memptr(), i0.data(), t1.memptr(), i1.data(), final_time, half_length, n_grid,
                               out.memptr(), n),
          dev.get(), "mi_restrict_f32_host");
}

// Several GPUs of one node behind the same call shapes (mi_group_*): contiguous query shards, the table
// replicated, one call per interpolation.  devices = {0, 1, ..}; a repeated ordinal rehearses the sharding on one GPU.
class DeviceGroup {
  public:
    explicit DeviceGroup(int ndev) : g_(nullptr) { check(mi_group_create(ndev, nullptr, &g_), nullptr, "mi_group_create"); }
    explicit DeviceGroup(const std::vector<int>& devices) : g_(nullptr)
    {
        check(mi_group_create((int)devices.size(), devices.data(), &g_), nullptr, "mi_group_create");
    }
    ~DeviceGroup() { mi_group_destroy(g_); }
    DeviceGroup(const DeviceGroup&) = delete;
    DeviceGroup& operator=(const DeviceGroup&) = delete;
    mi_group* get() const { return g_; }
    int size() const { return mi_group_size(g_); }

  private:
    mi_group* g_;
};

class GroupInterp1Table {
  public:
    GroupInterp1Table(DeviceGroup& grp, const arma::vec& X, const arma::vec& Y, bool sanitise = true) : grp_(grp), t_(nullptr)
    {
        if (X.n_elem != Y.n_elem) throw std::invalid_argument("interp1(): X and Y must have the same number of elements");
        check(mi_group_grid1_create(grp_.get(), X.memptr(), Y.memptr(), X.n_elem, sanitise ? MI_GRID_SANITISE : 0u, &t_), nullptr,
              "mi_group_grid1_create");
    }
    ~GroupInterp1Table() { mi_group_grid1_destroy(t_); }
    GroupInterp1Table(const GroupInterp1Table&) = delete;
    GroupInterp1Table& operator=(const GroupInterp1Table&) = delete;
    void operator()(const arma::vec& XI, arma::vec& YI, double extrap_val = std::numeric_limits<double>::quiet_NaN()) const
    {
        YI.set_size(XI.n_elem);
        check(mi_group_interp1_f64_host(grp_.get(), t_, XI.memptr(), YI.memptr(), XI.n_elem, extrap_val), nullptr,
              "mi_group_interp1_f64_host");
    }

  private:
    DeviceGroup& grp_;
    mi_group_grid1* t_;
};

// interp1 over the columns of a matrix with the columns sharded over the group (Interp1Axis; X and XI replicated)
class GroupInterp1Axis {
  public:
    GroupInterp1Axis(DeviceGroup& grp, const arma::vec& X) : grp_(grp), x_(X) {}
    void operator()(const arma::mat& Y, const arma::vec& XI, arma::mat& YI,
                    double extrap_val = std::numeric_limits<double>::quiet_NaN()) const
    {
        if (Y.n_rows != x_.n_elem) throw std::invalid_argument("interp1(): Y must have X.n_elem rows");
        YI.set_size(XI.n_elem, Y.n_cols);
        check(mi_group_interp1_cols_f64_host(grp_.get(), x_.memptr(), x_.n_elem, Y.memptr(), Y.n_rows, Y.n_cols, XI.memptr(),
                                             XI.n_elem, YI.memptr(), XI.n_elem, extrap_val),
              nullptr, "mi_group_interp1_cols_f64_host");
    }

  private:
    DeviceGroup& grp_;
    arma::vec x_;
};

// interp1 over paired columns with the columns sharded over the group (interp1_paired; XI replicated)
class GroupInterp1Paired {
  public:
    explicit GroupInterp1Paired(DeviceGroup& grp) : grp_(grp) {}
    void operator()(const arma::mat& X, const arma::mat& Y, const arma::vec& XI, arma::mat& YI,
                    double extrap_val = std::numeric_limits<double>::quiet_NaN(), std::vector<uint32_t>* ok = nullptr) const
    {
        if (X.n_rows != Y.n_rows || X.n_cols != Y.n_cols) throw std::invalid_argument("interp1_paired(): X and Y must have the same shape");
        YI.set_size(XI.n_elem, Y.n_cols);
        if (ok) ok->assign(Y.n_cols, 1u);
        check(mi_group_interp1_pairs_f64_host(grp_.get(), X.memptr(), X.n_rows, Y.memptr(), Y.n_rows, X.n_rows, nullptr, Y.n_cols,
                                              XI.memptr(), XI.n_elem, YI.memptr(), XI.n_elem, extrap_val,
                                              ok ? ok->data() : nullptr),
              nullptr, "mi_group_interp1_pairs_f64_host");
    }

  private:
    DeviceGroup& grp_;
};

// interp1 over paired columns with a query vector per column, the columns of X, Y and XI sharded over the group
class GroupInterp1Each {
  public:
    explicit GroupInterp1Each(DeviceGroup& grp) : grp_(grp) {}
    void operator()(const arma::mat& X, const arma::mat& Y, const arma::mat& XI, arma::mat& YI,
                    double extrap_val = std::numeric_limits<double>::quiet_NaN(), std::vector<uint32_t>* ok = nullptr) const
    {
        if (X.n_rows != Y.n_rows || X.n_cols != Y.n_cols) throw std::invalid_argument("interp1_each(): X and Y must have the same shape");
        if (XI.n_cols != X.n_cols) throw std::invalid_argument("interp1_each(): XI must have as many columns as X");
        YI.set_size(XI.n_rows, Y.n_cols);
        if (ok) ok->assign(Y.n_cols, 1u);
        check(mi_group_interp1_each_f64_host(grp_.get(), X.memptr(), X.n_rows, Y.memptr(), Y.n_rows, X.n_rows, nullptr, Y.n_cols,
                                             XI.memptr(), XI.n_rows, XI.n_rows, YI.memptr(), XI.n_rows, extrap_val,
                                             ok ? ok->data() : nullptr),
              nullptr, "mi_group_interp1_each_f64_host");
    }

  private:
    DeviceGroup& grp_;
};

// Bilinear interpolation over the group: Z = arma::mat(Y.n_elem, X.n_elem) replicated.  ZI an arma::vec: scattered
// (BASELINE config 3), the query pairs sharded, one result per pair; ZI an arma::mat: arma::interp2's gridded output,
// the columns of ZI sharded -- both as the mi355::interp2 overloads.
class GroupInterp2Table {
  public:
    GroupInterp2Table(DeviceGroup& grp, const arma::vec& X, const arma::vec& Y, const arma::mat& Z) : grp_(grp), t_(nullptr)
    {
        if (Z.n_rows != Y.n_elem || Z.n_cols != X.n_elem) throw std::invalid_argument("interp2(): Z must be Y.n_elem x X.n_elem");
        check(mi_group_grid2_create(grp_.get(), X.memptr(), X.n_elem, Y.memptr(), Y.n_elem, Z.memptr(), 0u, &t_), nullptr,
              "mi_group_grid2_create");
    }
    ~GroupInterp2Table() { mi_group_grid2_destroy(t_); }
    GroupInterp2Table(const GroupInterp2Table&) = delete;
    GroupInterp2Table& operator=(const GroupInterp2Table&) = delete;
    void operator()(const arma::vec& XI, const arma::vec& YI, arma::vec& ZI,
                    double extrap_val = std::numeric_limits<double>::quiet_NaN()) const
    {
        if (XI.n_elem != YI.n_elem) throw std::invalid_argument("interp2(): XI and YI must have the same number of elements");
        ZI.set_size(XI.n_elem);
        check(mi_group_interp2_f64_host(grp_.get(), t_, XI.memptr(), YI.memptr(), ZI.memptr(), XI.n_elem, extrap_val), nullptr,
              "mi_group_interp2_f64_host");
    }
    void operator()(const arma::vec& XI, const arma::vec& YI, arma::mat& ZI,
                    double extrap_val = std::numeric_limits<double>::quiet_NaN()) const
    {
        ZI.set_size(YI.n_elem, XI.n_elem);
        check(mi_group_interp2_grid_f64_host(grp_.get(), t_, XI.memptr(), XI.n_elem, YI.memptr(), YI.n_elem, ZI.memptr(),
                                             extrap_val),
              nullptr, "mi_group_interp2_grid_f64_host");
    }

  private:
    DeviceGroup& grp_;
    mi_group_grid2* t_;
};

}  // namespace mi355
