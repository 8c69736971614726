// swh_grec.h — the gpart record of a gspace: the one place that knows its
// fields. Every gspace kernel outside the gravity calls (the step, the
// statistics, the displacement sums, the gas link, the halo finder, the
// lightcone pass) takes its
// offsets, its checks and its loads and stores from here.
//
//   GRecLayout      the stride and every offset such a kernel uses, by value
//   grec_check      one field table, one check of a set of fields against the
//                   stride; the kNeed* sets say what each entry asks
//   grec_is_std     the whole multi-softening record (abi.GPART_DTYPE: 96
//                   bytes, every field from v_full on in bytes 32..96), whose
//                   bytes 32..96 a lane can move as four aligned 16-byte pieces
//                     q0 = v_full[0..3), a_grav[0]
//                     q1 = a_grav[1..3), a_grav_mesh[0..2)
//                     q2 = a_grav_mesh[2], potential, potential_mesh, mass
//                     q3 = old_a_grav_norm, epsilon, {time_bin, type, pad}, pad
//   GRec<STD>       (device) a record's fields in registers: STD by pieces,
//                   otherwise field by field through the checked offsets
//   grec_dispatch   the run-time "standard record" flag as a template argument
//   gspace_record   (library) what every entry asks of a gspace before it
//                   reads a record: upload, step layout, the fields it needs
//
// The part above __HIPCC__ needs no HIP header: the plain host programs of
// tests/test_coupled_host.py and tests/test_grec_host.py include it.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "swh_timeline.h"  // SWH_HD

namespace swh {

struct GRecLayout {
  int stride;
  int id;  // id_or_neg_offset: the first member of struct gpart in every gravity scheme
  int x, v_full, a_grav, a_grav_mesh, potential, potential_mesh, mass;
  int old_a_grav_norm;  // -1: not in the record (the adaptive MAC then sees 0)
  int epsilon, time_bin;
  int type;  // -1: no step layout set
};

// The fields as bits of a `need` set, in the order of kGRecFields.
enum : unsigned {
  GF_ID = 1u << 0, GF_X = 1u << 1, GF_V_FULL = 1u << 2, GF_A_GRAV = 1u << 3,
  GF_A_GRAV_MESH = 1u << 4, GF_POTENTIAL = 1u << 5, GF_POTENTIAL_MESH = 1u << 6,
  GF_MASS = 1u << 7, GF_OLD_A_GRAV_NORM = 1u << 8, GF_EPSILON = 1u << 9, GF_TIME_BIN = 1u << 10,
  GF_TYPE = 1u << 11
};

// The multi-softening record.
enum : int {
  kStdStride = 96, kStdId = 0, kStdX = 8, kStdVFull = 32, kStdAGrav = 44, kStdAGravMesh = 56,
  kStdPotential = 68, kStdPotentialMesh = 72, kStdMass = 76, kStdOldAGravNorm = 80,
  kStdEpsilon = 84, kStdTimeBin = 88, kStdType = 89
};
static_assert(kStdVFull % 16 == 0 && kStdStride == kStdVFull + 64 && kStdAGrav == kStdVFull + 12 &&
                  kStdAGravMesh == kStdAGrav + 12 && kStdPotential == kStdAGravMesh + 12 &&
                  kStdPotentialMesh == kStdPotential + 4 && kStdMass == kStdPotentialMesh + 4 &&
                  kStdOldAGravNorm == kStdMass + 4 && kStdEpsilon == kStdOldAGravNorm + 4 &&
                  kStdTimeBin == kStdEpsilon + 4 && kStdType == kStdTimeBin + 1,
              "the four 16-byte pieces of GRec<true>");

struct GRecField {
  const char* name;
  int GRecLayout::*off;
  int size, align;  // bytes
  int std_off;
  bool optional;    // a negative offset says "not in the record"
};
constexpr int kGRecNumFields = 12;
constexpr GRecField kGRecFields[kGRecNumFields] = {
    {"id_or_neg_offset", &GRecLayout::id, 8, 8, kStdId, false},
    {"x", &GRecLayout::x, 24, 8, kStdX, false},
    {"v_full", &GRecLayout::v_full, 12, 4, kStdVFull, false},
    {"a_grav", &GRecLayout::a_grav, 12, 4, kStdAGrav, false},
    {"a_grav_mesh", &GRecLayout::a_grav_mesh, 12, 4, kStdAGravMesh, false},
    {"potential", &GRecLayout::potential, 4, 4, kStdPotential, false},
    {"potential_mesh", &GRecLayout::potential_mesh, 4, 4, kStdPotentialMesh, false},
    {"mass", &GRecLayout::mass, 4, 4, kStdMass, false},
    {"old_a_grav_norm", &GRecLayout::old_a_grav_norm, 4, 4, kStdOldAGravNorm, true},
    {"epsilon", &GRecLayout::epsilon, 4, 4, kStdEpsilon, false},
    {"time_bin", &GRecLayout::time_bin, 1, 1, kStdTimeBin, false},
    {"type", &GRecLayout::type, 1, 1, kStdType, false},
};

// What each entry asks (the fields its kernels touch).
constexpr unsigned kNeedStepLayout = GF_V_FULL | GF_A_GRAV_MESH | GF_POTENTIAL_MESH | GF_TYPE;
constexpr unsigned kNeedStep = kNeedStepLayout | GF_X | GF_A_GRAV | GF_POTENTIAL | GF_EPSILON |
                               GF_TIME_BIN | GF_OLD_A_GRAV_NORM;
constexpr unsigned kNeedDriftSoftened = kNeedStep | GF_MASS;
constexpr unsigned kNeedStats = GF_X | GF_V_FULL | GF_A_GRAV | GF_A_GRAV_MESH | GF_POTENTIAL |
                                GF_MASS | GF_TIME_BIN | GF_TYPE;
constexpr unsigned kNeedRms = GF_V_FULL | GF_MASS | GF_TIME_BIN | GF_TYPE;
constexpr unsigned kNeedLink = GF_X | GF_V_FULL | GF_A_GRAV | GF_A_GRAV_MESH | GF_TIME_BIN | GF_TYPE;
constexpr unsigned kNeedFof = GF_X | GF_MASS | GF_TIME_BIN;  // and GF_TYPE with a step layout
// (and GF_ID for the check: the kernel reads id_or_neg_offset as swh_couple.h does)
constexpr unsigned kNeedLightcone = GF_X | GF_V_FULL | GF_MASS | GF_TIME_BIN | GF_TYPE;

// Every field of `need` lies inside the record, aligned to its type (an
// uploaded stride is a positive multiple of 8: make_glayout). Returns NULL, or
// the message of the first field that does not (valid until this thread's
// next call). `what` names the entry.
inline const char* grec_check(const GRecLayout& L, unsigned need, const char* what) {
  static thread_local char msg[192];
  for (int k = 0; k < kGRecNumFields; k++) {
    const GRecField& f = kGRecFields[k];
    if (!(need & (1u << k))) continue;
    const int off = L.*f.off;
    if (off < 0 && f.optional) continue;
    if (off >= 0 && off % f.align == 0 && (int64_t)off + f.size <= (int64_t)L.stride) continue;
    snprintf(msg, sizeof(msg), "%s: %s at byte %d (%d bytes, %d-byte aligned) must lie inside the "
             "gpart record of %d bytes", what, f.name, off, f.size, f.align, L.stride);
    return msg;
  }
  return nullptr;
}

// The whole multi-softening record, its first one (so every one) 16-byte aligned.
inline bool grec_is_std(const GRecLayout& L, const void* aos) {
  for (const GRecField& f : kGRecFields)
    if (L.*f.off != f.std_off) return false;
  return L.stride == kStdStride && reinterpret_cast<uintptr_t>(aos) % 16 == 0;
}

// f(std::true_type) or f(std::false_type): each launch is written once, as
//   grec_dispatch(std_rec, [&](auto STD) { launch kernel<decltype(STD)::value> });
template <typename F>
inline void grec_dispatch(bool std_rec, F&& f) {
  if (std_rec)
    f(std::true_type{});
  else
    f(std::false_type{});
}

}  // namespace swh

#ifdef __HIPCC__
#include "swh_internal.h"

namespace swh {

inline GRecLayout grec_layout(const GLayout& G, const swh_gpart_step_layout* S) {
  GRecLayout L;
  L.stride = G.stride;
  L.id = kStdId;
  L.x = G.x;
  L.v_full = S ? S->off_v_full : -1;
  L.a_grav = G.a_grav;
  L.a_grav_mesh = S ? S->off_a_grav_mesh : -1;
  L.potential = G.potential;
  L.potential_mesh = S ? S->off_potential_mesh : -1;
  L.mass = G.mass;
  L.old_a_grav_norm = G.old_a_grav_norm;
  L.epsilon = G.epsilon;
  L.time_bin = G.time_bin;
  L.type = S ? S->off_type : -1;
  return L;
}
inline GRecLayout grec_layout(const swh_gspace* g) {
  return grec_layout(g->layout, g->step_layout_set ? &g->step_layout : nullptr);
}

inline swh_status grec_require(const GRecLayout& L, unsigned need, const char* what) {
  const char* msg = grec_check(L, need, what);
  if (!msg) return SWH_OK;
  set_error("%s", msg);
  return SWH_ERR_ARG;
}

// The order every entry keeps: upload, step layout, then the offsets, so no
// kernel indexes a record with an offset that was not compared with the
// stride. An empty set asks nothing of its offsets.
inline swh_status gspace_record(const swh_gspace* g, unsigned need, const char* what,
                                GRecLayout* L) {
  if (!g->uploaded) {
    set_error("swh_gspace_upload must precede %s", what);
    return SWH_ERR_STATE;
  }
  if (!g->step_layout_set) {
    set_error("swh_gspace_set_step_layout must precede %s", what);
    return SWH_ERR_STATE;
  }
  *L = grec_layout(g);
  return g->n == 0 ? SWH_OK : grec_require(*L, need, what);
}

// The fields of each piece of the standard record.
constexpr unsigned kGPiece0 = GF_V_FULL | GF_A_GRAV, kGPiece1 = GF_A_GRAV | GF_A_GRAV_MESH,
                   kGPiece2 = GF_A_GRAV_MESH | GF_POTENTIAL | GF_POTENTIAL_MESH | GF_MASS,
                   kGPiece3 = GF_OLD_A_GRAV_NORM | GF_EPSILON | GF_TIME_BIN | GF_TYPE;

// A record's fields in registers. F, a constant, names the fields of a call:
//   load<F>         STD: the 16-byte pieces that hold them, and every field of
//                   those pieces; else load_fields<F>
//   load_fields<F>  each field by itself (STD: at the standard offsets, and
//                   time_bin with type as the one word that holds both)
//   store<F>        STD: the fields into the pieces that hold them, and those
//                   pieces whole, so load<> them first; else each field
// x goes as three doubles and a stored time_bin as its own byte either way.
template <bool STD>
struct GRec {
  double x[3];
  float v[3], a[3], am[3], pot, potm, mass, oagn, eps;
  int bin, type;
  float4 q0, q1, q2, q3;

  static __device__ __forceinline__ int at(int std_off, int off) { return STD ? std_off : off; }

  template <unsigned F>
  __device__ __forceinline__ void load_fields(const GRecLayout& L, const char* r) {
    static_assert(!(F & GF_ID), "swh_couple.h reads id_or_neg_offset");
    if (F & GF_X) load3(x, r + at(kStdX, L.x));
    if (F & GF_V_FULL) load3(v, r + at(kStdVFull, L.v_full));
    if (F & GF_A_GRAV) load3(a, r + at(kStdAGrav, L.a_grav));
    if (F & GF_A_GRAV_MESH) load3(am, r + at(kStdAGravMesh, L.a_grav_mesh));
    if (F & GF_POTENTIAL) pot = *reinterpret_cast<const float*>(r + at(kStdPotential, L.potential));
    if (F & GF_POTENTIAL_MESH)
      potm = *reinterpret_cast<const float*>(r + at(kStdPotentialMesh, L.potential_mesh));
    if (F & GF_MASS) mass = *reinterpret_cast<const float*>(r + at(kStdMass, L.mass));
    if (F & GF_OLD_A_GRAV_NORM)
      oagn = (STD || L.old_a_grav_norm >= 0)
                 ? *reinterpret_cast<const float*>(r + at(kStdOldAGravNorm, L.old_a_grav_norm))
                 : 0.f;
    if (F & GF_EPSILON) eps = *reinterpret_cast<const float*>(r + at(kStdEpsilon, L.epsilon));
    if (STD && (F & GF_TIME_BIN) && (F & GF_TYPE)) {
      bin_type(*reinterpret_cast<const int*>(r + kStdTimeBin));
    } else {
      if (F & GF_TIME_BIN) bin = *reinterpret_cast<const int8_t*>(r + at(kStdTimeBin, L.time_bin));
      if (F & GF_TYPE) type = *reinterpret_cast<const int8_t*>(r + at(kStdType, L.type));
    }
  }

  template <unsigned F>
  __device__ __forceinline__ void load(const GRecLayout& L, const char* r) {
    if (!STD) return load_fields<F>(L, r);
    load_fields<F & GF_X>(L, r);
    const float4* p = reinterpret_cast<const float4*>(r + kStdVFull);
    constexpr bool p0 = F & kGPiece0, p1 = F & kGPiece1, p2 = F & kGPiece2, p3 = F & kGPiece3;
    if (p0) q0 = p[0];
    if (p1) q1 = p[1];
    if (p2) q2 = p[2];
    if (p3) q3 = p[3];
    // every field the pieces hold, asked for or not
    if (p0) v[0] = q0.x, v[1] = q0.y, v[2] = q0.z;
    if (p0 && p1) a[0] = q0.w, a[1] = q1.x, a[2] = q1.y;
    if (p1 && p2) am[0] = q1.z, am[1] = q1.w, am[2] = q2.x;
    if (p2) pot = q2.y, potm = q2.z, mass = q2.w;
    if (p3) {
      oagn = q3.x, eps = q3.y;
      bin_type(__float_as_int(q3.z));
    }
  }

  template <unsigned F>
  __device__ __forceinline__ void store(const GRecLayout& L, char* r) {
    static_assert(!(F & ~(GF_X | GF_V_FULL | GF_A_GRAV | GF_POTENTIAL | GF_OLD_A_GRAV_NORM |
                          GF_EPSILON | GF_TIME_BIN)),
                  "no kernel writes the other fields");
    if (F & GF_X) store3(r + at(kStdX, L.x), x);
    if (F & GF_TIME_BIN)
      *reinterpret_cast<int8_t*>(r + at(kStdTimeBin, L.time_bin)) = (int8_t)bin;
    if (STD) {
      if (F & GF_V_FULL) q0.x = v[0], q0.y = v[1], q0.z = v[2];
      if (F & GF_A_GRAV) q0.w = a[0], q1.x = a[1], q1.y = a[2];
      if (F & GF_POTENTIAL) q2.y = pot;
      if (F & GF_OLD_A_GRAV_NORM) q3.x = oagn;
      if (F & GF_EPSILON) q3.y = eps;
      constexpr unsigned P = F & ~(GF_X | GF_TIME_BIN);
      float4* p = reinterpret_cast<float4*>(r + kStdVFull);
      if (P & kGPiece0) p[0] = q0;
      if (P & kGPiece1) p[1] = q1;
      if (P & kGPiece2) p[2] = q2;
      if (P & kGPiece3) p[3] = q3;
    } else {
      if (F & GF_V_FULL) store3(r + L.v_full, v);
      if (F & GF_A_GRAV) store3(r + L.a_grav, a);
      if (F & GF_POTENTIAL) *reinterpret_cast<float*>(r + L.potential) = pot;
      if ((F & GF_OLD_A_GRAV_NORM) && L.old_a_grav_norm >= 0)
        *reinterpret_cast<float*>(r + L.old_a_grav_norm) = oagn;
      if (F & GF_EPSILON) *reinterpret_cast<float*>(r + L.epsilon) = eps;
    }
  }

 private:
  // the word at kStdTimeBin: time_bin, type, padding
  __device__ __forceinline__ void bin_type(int bits) {
    bin = (int)(int8_t)(bits & 0xff);
    type = (int)(int8_t)((bits >> 8) & 0xff);
  }
  template <typename T>
  static __device__ __forceinline__ void load3(T (&o)[3], const char* p) {
    const T* f = reinterpret_cast<const T*>(p);
    o[0] = f[0], o[1] = f[1], o[2] = f[2];
  }
  template <typename T>
  static __device__ __forceinline__ void store3(char* p, const T (&o)[3]) {
    T* f = reinterpret_cast<T*>(p);
    f[0] = o[0], f[1] = o[1], f[2] = o[2];
  }
};

}  // namespace swh
#endif  // __HIPCC__
