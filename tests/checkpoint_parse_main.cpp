// checkpoint_parse_main.cpp -- a stand-alone driver of the checkpoint blob's parser (rayfinder_amd/csrc/rf_checkpoint.cpp), built by tests/test_checkpoint_api.py with
// -fsanitize=address,undefined and run as a plain executable.
//   checkpoint_parse_main GOOD [BAD ...]
// GOOD must parse, and every array entry the parser hands out is then read (so that an offset past the blob would be seen); every BAD must be refused with
// std::invalid_argument; then 256 seeded single-byte corruptions of GOOD's header must each parse or be refused -- nothing else.  Every blob is parsed from a heap
// copy of exactly its size.  Exit 0: all of that held.
#include "rf_checkpoint.hpp"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>

namespace
{
std::vector<unsigned char> readFile(const char* path)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) std::fprintf(stderr, "cannot open %s\n", path), std::exit(2);
    return std::vector<unsigned char>(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
}

// 0: parsed (and walked), 1: refused with std::invalid_argument
int tryParse(const std::vector<unsigned char>& bytes)
{
    // an exact-size heap copy: one byte past the end is the sanitizer's
    std::unique_ptr<unsigned char[]> copy(new unsigned char[bytes.size() ? bytes.size() : 1]);
    std::copy(bytes.begin(), bytes.end(), copy.get());
    try
    {
        const rf::ckpt::View v = rf::ckpt::parse(copy.get(), bytes.size());
        uint64_t             sink = 0;
        for (uint32_t k = 0; k < v.header.numTiles; ++k)
        {
            sink += v.tileId(k) + v.tileSamples(k);
            for (uint32_t p = 0; p < v.numPlanes; ++p)
            {
                sink += v.tileDigest(p, k);
                const unsigned char* tile = v.planeTile(p, k);
                sink += tile[0] + tile[rf::ckpt::kTileTexels * rf::ckpt::kTexelBytes - 1];
            }
        }
        if (sink == 0x5EEDFACEull) std::puts("");
        return 0;
    }
    catch (const std::invalid_argument&)
    {
        return 1;
    }
}
} // namespace

int main(int argc, char** argv)
{
    if (argc < 2) return std::fprintf(stderr, "usage: %s GOOD [BAD ...]\n", argv[0]), 2;
    const std::vector<unsigned char> good = readFile(argv[1]);
    if (tryParse(good) != 0) return std::fprintf(stderr, "the good blob was refused\n"), 1;
    for (int i = 2; i < argc; ++i)
        if (tryParse(readFile(argv[i])) != 1) return std::fprintf(stderr, "%s was not refused\n", argv[i]), 1;
    uint64_t state = 0x243F6A8885A308D3ull;
    int      parsed = 0, refused = 0;
    for (int i = 0; i < 256; ++i)
    {
        state = rf::ckpt::mix64(state + 0x9E3779B97F4A7C15ull * static_cast<uint64_t>(i + 1));
        std::vector<unsigned char> bad = good;
        const size_t               at = static_cast<size_t>(state % rf::ckpt::kHeaderBytes);
        bad[at] ^= static_cast<unsigned char>(1u << ((state >> 32) % 8u));
        (tryParse(bad) == 0 ? parsed : refused) += 1;
    }
    std::printf("good parsed, %d bad refused, corruptions: %d parsed, %d refused\n", argc - 2, parsed, refused);
    return 0;
}
