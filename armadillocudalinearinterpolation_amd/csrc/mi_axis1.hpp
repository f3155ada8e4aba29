// The validated 1-D axis handle (mi_axis1_create, mi_cols1.hip), shared by the calls that take one: interp1 over the
// columns of a matrix (mi_cols1.hip) and interp2 over the slices of a cube (mi_slices2.hip).
#pragma once
#include "mi_interp2_eval.hpp"

struct mi_axis1 {
    mi_ctx* ctx;
    int device;            // copied at creation: destroy must not dereference a context that may be gone
    void* dev_x;           // explicit nodes (null for a uniform axis)
    AxisDev a;
    size_t n;
};
