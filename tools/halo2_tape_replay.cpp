// Validates and replays a Halo2 witness tape on the host, without Python and without a device: the stand-alone program the host side of the
// tape (halo2_tape_validate, halo2_replay_host) is run under sanitizers with.
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       -I stark-verifier_amd/csrc tools/halo2_tape_replay.cpp stark-verifier_amd/csrc/halo2_synth_host.cpp -o halo2_tape_replay
//   halo2_tape_replay TAPE_FILE
// The file is 64-bit little-endian words: k, the number of inputs, the number of tape words, the tape, the inputs -- from a Recorder `rec`:
//   np.concatenate([np.array([rec.k, len(rec.inputs), rec.tape().size], dtype="<u8"), rec.tape(), np.array(rec.inputs, dtype="<u8")]).tofile(path)
// Prints the status and a checksum of the columns;
// exit status 0 when the tape is valid (whether or not an entry fails), 2 when the validator refuses it, 1 for a file it cannot read.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "halo2_tape.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s TAPE_FILE\n", argv[0]); return 1; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    uint64_t head[3];
    if (fread(head, 8, 3, f) != 3 || head[0] > 28 || head[1] > (1ull << 32) || head[2] > (1ull << 36)) { fprintf(stderr, "%s: not a tape file\n", argv[1]); fclose(f); return 1; }
    const uint32_t k = (uint32_t)head[0];
    std::vector<uint64_t> tape(head[2]), inputs(head[1]);
    const bool whole = fread(tape.data(), 8, tape.size(), f) == tape.size() && fread(inputs.data(), 8, inputs.size(), f) == inputs.size();
    fclose(f);
    if (!whole) { fprintf(stderr, "%s: truncated\n", argv[1]); return 1; }
    std::vector<uint64_t> level_start;
    if (const char* what = gl355::halo2_tape_validate(tape.data(), tape.size(), inputs.size(), k, gl355::H2_N_ADVICE, &level_start)) {
        printf("refused: %s\n", what);
        return 2;
    }
    std::vector<uint64_t> advice((size_t)gl355::H2_N_ADVICE * 4 << k);
    uint64_t status[2];
    gl355::halo2_replay_host(tape.data(), tape.size() / gl355::H2_ENTRY_WORDS, k, inputs.data(), advice.data(), status);
    uint64_t sum = 0;
    for (uint64_t w : advice) sum = sum * 0x100000001B3ull + w;
    printf("k %u  entries %zu  levels %zu  first failing entry %lld  failing entries %llu  columns %016llx\n", k, tape.size() / gl355::H2_ENTRY_WORDS,
           level_start.size() - 1, (long long)status[0], (unsigned long long)status[1], (unsigned long long)sum);
    return 0;
}
