// host_scene.hpp — what a p3d_host_scene handle holds.  Private to the host translation units: host_capi.cpp, which loads,
// edits and flattens it, and host_queries.cpp, which states the queries on it.
#pragma once
#include "accel_build.hpp"
#include "p3d.h"
#include "scene_model.hpp"

struct p3d_host_scene {
  p3d::Scene scene;
  std::unique_ptr<p3d::BVH> bvh;
  std::unique_ptr<p3d::Grid> grid;
  std::vector<p3d_prim> prims;
  std::vector<p3d_material> materials;
  std::vector<p3d_light> lights;
  p3d_scene_desc desc{};
  bool flat_valid = false;
};
