// host_check.cpp -- CPU-only build of the host code that reads untrusted input (ttsw_host.h), for the sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all host_check.cpp -o ttsw_check_asan
// (csrc/build_host_asan.sh; GPU AddressSanitizer is not available on the pool, and this code needs no GPU).
// usage: ttsw_check_asan [--load] file...   -- one line per file: "<status> <tensors> <floats> <message>"; --load also reads
// every payload (what tts_hip_load_weights does), without it only the container is validated (tts_hip_check_weights_file).
//        ttsw_check_asan --wg-plan LO HI [STEP]  -- the WaveGlow dispatch (wg_plan.h), one line "BT precision form PR tiles
// wino_wanted" for every STEP-th (default: every) frame count LO..HI, the three precisions and forms 0..3
// (tests/test_wg_plan.py compares them with pick_variant).
// Exit status 0 unless a sanitizer aborts the process.
#include <cstdlib>

#include "ttsw_host.h"
#include "wg_plan.h"

static int print_wg_plans(int lo, int hi, int step) {
    for (int bt = lo; bt <= hi; bt += step)
        for (int precision = 0; precision < 3; ++precision)
            for (int form = 0; form < 4; ++form) {
                const WgPlan p = wg_plan(bt, precision, form);
                if (p.BT != bt || p.M != 32ll * p.PR || p.NP != (precision == 2 ? 2 : 1)) return 2;
                printf("%d %d %d %d %d %d\n", bt, precision, form, p.PR, (int)p.tiles, (int)p.wino_wanted);
            }
    return 0;
}

int main(int argc, char** argv) {
    if ((argc == 4 || argc == 5) && !strcmp(argv[1], "--wg-plan")) {
        const int step = argc == 5 ? atoi(argv[4]) : 1;
        return step > 0 ? print_wg_plans(atoi(argv[2]), atoi(argv[3]), step) : 2;
    }
    bool load = false;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--load")) {
            load = true;
            continue;
        }
        std::map<std::string, HostTensor> tensors;
        std::string err;
        const int rc = parse_ttsw(argv[i], load ? &tensors : nullptr, &err);
        size_t floats = 0;
        for (auto& kv : tensors) {
            floats += kv.second.data.size();
            if (kv.second.numel() != kv.second.data.size()) return 2;          // dims and payload must agree after a load
        }
        printf("%d %zu %zu %s\n", rc, tensors.size(), floats, err.c_str());
    }
    return 0;
}
