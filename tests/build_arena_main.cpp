// The sweep of tests/build_arena_shim.cpp as a program of its own, for a build with -fsanitize=address,undefined:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nrays_amd/csrc -o build_arena_sweep tests/build_arena_main.cpp tests/build_arena_shim.cpp
#include <cstdint>
#include <cstdio>

extern "C" uint64_t build_arena_sweep(uint64_t* cases);

int main() {
    uint64_t cases = 0;
    const uint64_t bad = build_arena_sweep(&cases);
    std::printf("build_arena sweep: %llu cases, %llu unsound\n", (unsigned long long)cases, (unsigned long long)bad);
    return bad || !cases ? 1 : 0;
}
