// query_refusals.hpp — the refusals that the host forms of the per-object queries (host_queries.cpp) and their device entry
// points (csrc/capi_proximity.hpp) word alike, in ONE place for both.  Each is what follows the entry point's "p3d_...: " prefix.
#pragma once
#include <string>

#include "p3d.h"

namespace p3d {

static_assert(P3D_NEAREST_K_MAX == 16 && P3D_FILTER_SKIP_MAX == 8, "the texts below spell the limits out");

constexpr const char* kRefuseNearestK = "k must be 1 .. P3D_NEAREST_K_MAX (16)";
constexpr const char* kRefuseOverlapK = "k must be 0 .. P3D_NEAREST_K_MAX (16)";  // (0: the count alone)
constexpr const char* kRefuseSkipCount = "n_skip must be 0 .. P3D_FILTER_SKIP_MAX (8)";
constexpr const char* kRefuseOverlapFlag = "unknown flag (P3D_OVERLAP_SOLID is the only one)";
constexpr const char* kRefusePlaneUnderTree =
    "the scene holds a plane, whose box in the BVH is the [-1,1]^3 default: the tree cannot find it (use P3D_ACCEL_NONE)";
// why a query that does not take boxes refuses a scene that holds one: the sphere sweep's sentence, and the segment query's
constexpr const char* kSweepNoBox = "a ball against a box (a rounded box, and its inside) is not swept";
constexpr const char* kSegmentNoBox = "a segment against a box's faces is not part of this query";

inline std::string refuse_box(int object, const char* why) { return "object " + std::to_string(object) + " is a box: " + why; }

}  // namespace p3d
