// scene_file.hpp -- the raw scene file the host-only test programs read (tests/scene_pack_main.cpp, tests/launch_policy_main.cpp; its writer: tests/scene_pack_scenes.py).
// "RFSCENE1", u64 nodes, u64 triangles, u64 textures, then the 48-byte nodes, the 48-byte position attributes, the 80-byte vertex attributes and per texture
// {u32 width, u32 height, width * height u32 texels}.  Include rf_bvh.hpp first (rf::SceneView and the records).
#pragma once

#include <cstdint>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace
{
struct SceneFile
{
    std::vector<rf::BvhNode>               nodes;
    std::vector<rf::PositionAttribute>     positions;
    std::vector<rf::VertexAttributes>      attributes;
    std::vector<std::vector<uint32_t>>     texels;
    std::vector<rf::TextureView>           textures;
    rf::SceneView view() const { return {nodes, positions, attributes, textures}; }
};

template<typename T>
void readArray(std::ifstream& in, std::vector<T>& out, uint64_t count, uint64_t bytesLeft)
{
    if (count > bytesLeft / sizeof(T)) throw std::runtime_error("scene file: an array is longer than the file");
    out.resize(count);
    in.read(reinterpret_cast<char*>(out.data()), static_cast<std::streamsize>(count * sizeof(T)));
    if (!in) throw std::runtime_error("scene file: truncated");
}

SceneFile readScene(const std::string& path)
{
    std::ifstream in(path, std::ios::binary | std::ios::ate);
    if (!in) throw std::runtime_error("scene file: cannot open " + path);
    const uint64_t size = static_cast<uint64_t>(in.tellg());
    in.seekg(0);
    char     magic[8];
    uint64_t counts[3];
    in.read(magic, 8);
    in.read(reinterpret_cast<char*>(counts), sizeof counts);
    if (!in || std::memcmp(magic, "RFSCENE1", 8) != 0) throw std::runtime_error("scene file: bad header");
    SceneFile s;
    readArray(in, s.nodes, counts[0], size);
    readArray(in, s.positions, counts[1], size);
    readArray(in, s.attributes, counts[1], size);
    if (counts[2] > size / 8) throw std::runtime_error("scene file: more textures than the file holds");
    s.texels.resize(counts[2]);
    for (auto& px : s.texels)
    {
        uint32_t wh[2];
        in.read(reinterpret_cast<char*>(wh), sizeof wh);
        if (!in) throw std::runtime_error("scene file: truncated");
        readArray(in, px, static_cast<uint64_t>(wh[0]) * wh[1], size);
        s.textures.push_back({px.data(), wh[0], wh[1]});
    }
    return s;
}
} // namespace
