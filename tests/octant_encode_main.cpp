// Drives csrc/host/scene_encode.cpp alone (tests/test_octant_encode.py): reads a two-triangle scene
// with a hand-made tree from the file named on the command line -- int32 nv, nn, then nv float4
// vertices and nn 48-byte BVH nodes -- encodes it and prints the fast-quotient flag.
#include <cstdio>
#include <string>
#include <vector>

#include "rt_abi.h"
#include "scene_encode.hpp"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t nv = 0, nn = 0;
    if (std::fread(&nv, 4, 1, f) != 1 || std::fread(&nn, 4, 1, f) != 1 || nv < 3 || nv % 3 || nv > 300 || nn < 1 || nn > 300)
        return 2;
    std::vector<rt_float4> verts(nv);
    std::vector<rt_bvh_node> nodes(nn);
    if (std::fread(verts.data(), sizeof(rt_float4), nv, f) != (size_t)nv ||
        std::fread(nodes.data(), sizeof(rt_bvh_node), nn, f) != (size_t)nn)
        return 2;
    std::fclose(f);
    // every triangle its own vertices and reference, one normal, one material
    std::vector<int32_t> idx(nv), normal_idx(nv, 0), refs(nv / 3), tri_to_mat(nv / 3, 0);
    for (int32_t i = 0; i < nv; ++i) idx[i] = i;
    for (int32_t t = 0; t < nv / 3; ++t) refs[t] = 3 * t;
    const rt_float4 normal{0.0f, 1.0f, 0.0f, 0.0f};
    const rt_material mat{};
    rtamd::EncodedScene e;
    std::string err;
    const int rc = rtamd::encode_scene(verts.data(), nv, idx.data(), nv, nodes.data(), nn, refs.data(), (int32_t)refs.size(),
                                       &normal, 1, normal_idx.data(), &mat, 1, tri_to_mat.data(), e, err);
    if (rc != RT_OK) {
        std::printf("refused: %s\n", err.c_str());
        return 1;
    }
    std::printf("fast_div=%d clean=%d n_inner=%u\n", e.fast_div, e.clean, e.n_inner);
    return 0;
}
