// Heightfield lookup of the rigid-body simulator's terrain (sim_dynamics.h includes this and builds the contact law on it), as
// plain C++ on doubles: no device intrinsics, so the same text is compiled into sim_kernel.hip and into a stand-alone host
// program (tests/test_sim_terrain_cpu.py builds one under the address and undefined-behaviour sanitizers).
//
// Field: heights H[rows][cols] in C order, rows, cols >= 2; vertex (r, c) lies at world x = x0 + c dx, y = y0 + r dy, dx, dy > 0.
// Every cell is cut into two triangles by the diagonal from (r, c) to (r+1, c+1); the surface is the plane of the triangle the
// query point lies over.  Outside the field the surface continues as the CLAMPED point of the edge cell (fu, fv pinned to 0 or
// 1): a flat shelf at the edge's height with the edge triangle's slope as its normal -- unphysical, documented, never a fault.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define QRW_TERRAIN_FN __host__ __device__ __forceinline__
#else
#define QRW_TERRAIN_FN inline
#endif

namespace qrw {
namespace terrain {

struct Field {
  const double* H;  // [rows][cols]
  int rows, cols;
  double x0, y0, dx, dy;
};

// The cell under a query coordinate: index in 0 .. n-2 and the fraction in [0, 1] (NaN for a NaN coordinate).
// Clamped in double BEFORE the conversion to an integer: a huge, infinite or NaN coordinate gives an in-range index (NaN: 0),
// never an undefined conversion.  The fraction keeps a NaN, so that a NaN foot gives a non-finite force (the status freeze).
struct Axis {
  int i;
  double f;
};
QRW_TERRAIN_FN Axis axis_cell(double coord, double origin, double step, int n) {
  const double u = (coord - origin) / step;
  const double hi = (double)(n - 2);
  double t = floor(u);
  t = !(t >= 0.0) ? 0.0 : (t > hi ? hi : t);  // (a NaN fails `>= 0`)
  Axis a;
  a.i = (int)t;
  const double f = u - t;
  a.f = f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);
  return a;
}

// the four corners of cell (r, c): h00 = H[r][c], h10 = H[r][c+1], h01 = H[r+1][c], h11 = H[r+1][c+1]
struct Corners {
  double h00, h10, h01, h11;
};
QRW_TERRAIN_FN Corners load_corners(const Field& T, int r, int c) {
  const double* p = T.H + (size_t)r * (size_t)T.cols + (size_t)c;
  Corners k;
  k.h00 = p[0]; k.h10 = p[1];
  k.h01 = p[T.cols]; k.h11 = p[T.cols + 1];
  return k;
}

// height and gradient of the triangle (fu, fv) lies over
struct Plane {
  double h, gx, gy;
};
// (written with selects, not branches: all four corners are read whatever the triangle, so that the kernel's loads do not wait
// for the comparison -- a branch here made the compiler load the third corner inside it, one exposed latency after the other.
//  fu >= fv: h = h00 + fu (h10 - h00) + fv (h11 - h10), gx = (h10 - h00)/dx, gy = (h11 - h10)/dy
//  else    : h = h00 + fv (h01 - h00) + fu (h11 - h01), gx = (h11 - h01)/dx, gy = (h01 - h00)/dy)
QRW_TERRAIN_FN Plane plane_of(const Corners& k, double fu, double fv, double dx, double dy) {
  const bool lower = fu >= fv;
  const double mid = lower ? k.h10 : k.h01;           // the triangle's corner off the diagonal
  const double e0 = mid - k.h00, e1 = k.h11 - mid;    // the rise along its first and its second edge from (r, c)
  Plane s;
  s.h = k.h00 + (lower ? fu : fv) * e0 + (lower ? fv : fu) * e1;
  s.gx = (lower ? e0 : e1) / dx;
  s.gy = (lower ? e1 : e0) / dy;
  return s;
}

// the whole lookup at the world point (X, Y)
QRW_TERRAIN_FN Plane surface(const Field& T, double X, double Y) {
  const Axis u = axis_cell(X, T.x0, T.dx, T.cols), v = axis_cell(Y, T.y0, T.dy, T.rows);
  return plane_of(load_corners(T, v.i, u.i), u.f, v.f, T.dx, T.dy);
}

}  // namespace terrain
}  // namespace qrw
