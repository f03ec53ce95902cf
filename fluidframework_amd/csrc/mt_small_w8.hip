/* k_replay of the config 2/3 profile (HotSmall) built for 8 waves per SIMD (the 4-wave build: mt_small_w4.hip) */
#include "mt_kernels.h"

/* without snapshot-load records (Replica LOAD = false): the engine's default config-2/3 kernel */
int32_t replay_small_w8(mt_engine* e) {
    return launch_replay<HotSmall>(e, k_replay<HotSmall, false, 8, 1, false, false>);
}
