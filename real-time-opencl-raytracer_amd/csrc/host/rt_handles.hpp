// rt_handles.hpp -- the opaque handles of include/rt_host.h, for the host sources that define
// entry points over them (rt_host_abi.cpp, lbvh_builder.cpp).
#pragma once

#include "rt_host.h"
#include "scene.hpp"

struct rt_mesh { rtamd::Mesh m; };
struct rt_bvh { rtamd::Bvh b; };
