// refit.hpp -- the BVH refit plan shared by rt_refit_nodes (CPU) and rt_upload_scene /
// rt_update_vertices (device): which scenes can be refitted, and the bottom-up order.
// Plain C++ over the ABI structs; no HIP, and nothing else of csrc/host.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "rt_abi.h"

namespace rtrefit {

// A scene is refittable when every reachable node with offset_left >= 0 is a valid inner node
// and every reachable node has exactly one parent (the root none): the reachable nodes then
// form a tree, and every box has one writer.
struct Plan {
    std::vector<int32_t> order;         // reachable nodes, every parent before its children
    std::vector<uint32_t> ids;          // inner nodes grouped by height (longest path down to a leaf), 1 first
    std::vector<uint32_t> level_begin;  // ids of height h are ids[level_begin[h-1] .. level_begin[h]); H + 1 entries
    uint32_t heights() const { return level_begin.empty() ? 0u : (uint32_t)level_begin.size() - 1u; }
};

// Builds the plan of nodes[0..nn) (root 0; leaves' triangle ranges checked against nref).
// inner_id (nn entries) maps a node to the id its record has on the device (rt_upload_scene's
// numbering); NULL: the node's own index.  RT_OK, or RT_ERR_BAD_SCENE with `err` naming the node.
int plan_build(const rt_bvh_node* nodes, int32_t nn, int32_t nref, const int32_t* inner_id, Plan& plan,
               std::string& err);

// Message of the last failed rt_refit_nodes (empty after a successful one).
const std::string& last_error();
void clear_error();

}  // namespace rtrefit
