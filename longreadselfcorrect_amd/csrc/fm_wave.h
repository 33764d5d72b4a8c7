// fm_wave.h -- what a wavefront is to the tools that give one a read, a pair or a walk (fm_kcorrect.h, fm_fmwalk.h): the `W` that
// their per-read code is written against, and its plain definition.
//
// A `W` runs phases.  A phase is every lane's call, after which all lanes see what any of them wrote:
//
//   each(f)          f(lane) for the kWaveLanes lanes
//   min_over(f)      the same; every lane gets the smallest f(lane) (kWaveNone when every lane returns that)
//   sum_over(f)      the same; every lane gets the sum of f(lane), in 32 bits
//   sum64_over(f)    the same, in 64 bits
//   scan(f, g)       f(lane) for every lane, then g(lane, the sum of f over the lanes before it, f(lane)); every lane gets the
//                    sum over all
//
// Everything outside a phase is the same in every lane; uniform(v) and uniform64(v) say so of a value that was read from the
// state the lanes share, so that the device may keep it in scalar registers.  Nothing may depend on the order in which the lanes
// of a phase run.
//
// SerialWave is the definition: the lanes one after the other.  The device's W is fm_launch.h's WaveExec.  This header is free
// of HIP types: the drivers under tests/host_tools run the tools' code through SerialWave on the CPU.
#pragma once
#include <stdint.h>

namespace lrsc {

constexpr uint32_t kWaveLanes = 64;
constexpr uint32_t kWaveNone = 0xFFFFFFFFu;                       // min_over's identity: "no lane has anything"

struct SerialWave {
    static uint32_t uniform(uint32_t v) { return v; }
    static uint64_t uniform64(uint64_t v) { return v; }
    template <class F> void each(F&& f)
    {
        for(uint32_t lane = 0; lane < kWaveLanes; ++lane) f(lane);
    }
    template <class F> uint32_t min_over(F&& f)
    {
        uint32_t v = kWaveNone;
        for(uint32_t lane = 0; lane < kWaveLanes; ++lane) {
            const uint32_t x = f(lane);
            v = x < v ? x : v;
        }
        return v;
    }
    template <class F> uint32_t sum_over(F&& f)
    {
        uint32_t v = 0;
        for(uint32_t lane = 0; lane < kWaveLanes; ++lane) v += f(lane);
        return v;
    }
    template <class F> uint64_t sum64_over(F&& f)
    {
        uint64_t v = 0;
        for(uint32_t lane = 0; lane < kWaveLanes; ++lane) v += f(lane);
        return v;
    }
    template <class F, class G> uint32_t scan(F&& f, G&& g)
    {
        uint32_t mine[kWaveLanes], before = 0;
        for(uint32_t lane = 0; lane < kWaveLanes; ++lane) mine[lane] = f(lane);
        for(uint32_t lane = 0; lane < kWaveLanes; ++lane) {
            g(lane, before, mine[lane]);
            before += mine[lane];
        }
        return before;
    }
};

} // namespace lrsc
