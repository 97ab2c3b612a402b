#include "rf_gltf.hpp"
#include "rf_pt_format.hpp"
#include "rf_bvh_gpu.hpp"
#include "rf_scene_pack.hpp"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
namespace rf { Bvh buildBvhGpu(std::span<const Positions>, int, float*) { throw std::runtime_error("no gpu"); } }
int main(int argc, char** argv)
{
    int ok = 0, err = 0;
    for (int i = 1; i < argc; ++i)
    {
        const std::string path = argv[i];
        try
        {
            if (path.size() > 3 && path.substr(path.size() - 3) == ".pt")
            {
                // what rf_renderer_create does on the host with a scene that passed the reader: the structural check, then the packing itself
                // (every record layout, the leaf boxes, the shading records, the texture blob)
                auto f = rf::readPtFile(path);
                if (f.bvhNodes.empty() || f.trianglePositionAttributes.size() != f.triangleVertexAttributes.size()) { ++err; continue; }
                rf::validateScene(f.bvhNodes, f.trianglePositionAttributes.size(), f.triangleVertexAttributes, f.baseColorTextures.size());
                std::vector<rf::TextureView> textures;
                for (const rf::Texture& t : f.baseColorTextures) textures.push_back({t.pixels.data(), t.width, t.height});
                const rf::PackedScene packed = rf::packScene({f.bvhNodes, f.trianglePositionAttributes, f.triangleVertexAttributes, textures});
                ok += !packed.wide.nodes.empty() + (packed.texels.size() & 0);
            }
            else { auto f = rf::ptFormatFromGltf(path); ok += !f.bvhNodes.empty(); }
        }
        catch (const std::exception&) { ++err; }
    }
    std::printf("ok %d err %d\n", ok, err);
}
