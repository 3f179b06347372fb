// The sweep of tests/batch_stage_shim.cpp as a program of its own, for a build with -fsanitize=address,undefined:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nrays_amd/csrc -o batch_stage_sweep tests/batch_stage_main.cpp tests/batch_stage_shim.cpp
#include <cstdint>
#include <cstdio>

extern "C" uint64_t batch_stage_sweep(uint64_t* cases);

int main() {
    uint64_t cases = 0;
    const uint64_t bad = batch_stage_sweep(&cases);
    std::printf("batch_stage sweep: %llu cases, %llu unsound\n", (unsigned long long)cases, (unsigned long long)bad);
    return bad || !cases ? 1 : 0;
}
