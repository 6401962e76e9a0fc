// Stand-alone probe of artspeech_amd/csrc/operand_image.h for tests/test_operand_image_cpu.py (compiled there with g++, plain and under
// AddressSanitizer + UBSan): for every (K, N) on the command line's grid it fills a buffer of the header's image size by walking
// (group, part, column, entry) through the header's index function -- every int16 gets the code of its (k, part, column) --, appends
// the buffer to the file named by argv[1] and prints one JSON line: the header's kbx and size, whether the walk visited every int16 of
// the image exactly once, and whether the byte-offset form is 16 x the element form everywhere.
#include "operand_image.h"

#include <cstdio>
#include <vector>

namespace oi = operand_image;

static int16_t code(int k, int p, int j) { return (int16_t)(((k * 311 + j) * 2 + p) % 32003); }

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* out = std::fopen(argv[1], "wb");
    if (!out) return 2;
    const int Ks[] = {1, 8, 10, 16, 17, 64, 65, 130}, Ns[] = {0, 1, 63, 64, 65, 300};
    for (int K : Ks)
        for (int N : Ns) {
            const size_t bytes = oi::bytes(K, N), NX = oi::rows(N);
            std::vector<int16_t> img(bytes / 2, (int16_t)-1);
            std::vector<unsigned char> seen(bytes / 2, 0);
            bool once = true, off16 = true;
            size_t visited = 0;
            if (bytes)
                for (int g = 0; g < 2 * oi::kbx(K); ++g)
                    for (int p = 0; p < 2; ++p)
                        for (int j = 0; j <= N; ++j) {
                            const size_t row = oi::row(g, p, (size_t)j, NX);
                            off16 = off16 && oi::byte_off(oi::plane(g, p), (unsigned)j, oi::rows32(N)) == 16 * row &&
                                    row == oi::row_of(g >> 1, p, g & 1, (size_t)j, NX);
                            for (int r = 0; r < 8; ++r, ++visited) {
                                const size_t at = row * 8 + r;                 // (.at(): an index outside the image ends the probe)
                                once = once && !seen.at(at);
                                seen.at(at) = 1;
                                img.at(at) = code(8 * g + r, p, j);
                            }
                        }
            once = once && visited == bytes / 2;
            if (bytes && std::fwrite(img.data(), 2, img.size(), out) != img.size()) return 2;
            std::printf("{\"K\": %d, \"N\": %d, \"kbx\": %d, \"bytes\": %zu, \"desc_bytes\": %u, \"once\": %s, \"off16\": %s}\n", K, N, oi::kbx(K),
                        bytes, oi::desc_bytes(K, oi::rows32(N)), once ? "true" : "false", off16 ? "true" : "false");
        }
    return std::fclose(out) == 0 ? 0 : 2;
}
