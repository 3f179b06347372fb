// The cases of tests/host_scene_shim.cpp as a program of its own, for a build with -fsanitize=address,undefined (every case is flattened twice and the two reports compared):
//   g++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I nrays_amd/csrc -pthread -o host_scene_sweep \
//       tests/host_scene_main.cpp tests/host_scene_shim.cpp nrays_amd/csrc/scene_build.cpp nrays_amd/csrc/bvh_build.cpp nrays_amd/csrc/switches.cpp
#include <cstdio>

extern "C" int host_scene_sweep(int* cases);

int main() {
    int cases = 0;
    const int bad = host_scene_sweep(&cases);
    std::printf("host_scene sweep: %d cases, %d not deterministic\n", cases, bad);
    return bad || !cases ? 1 : 0;
}
