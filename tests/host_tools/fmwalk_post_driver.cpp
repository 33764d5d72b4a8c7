// fmwalk_post_driver.cpp -- `stride fmwalk --validate`'s post-processor (host/FMIndexWalkProcess.cpp) on results given as text, so that
// its three files and its summary lines can be checked where there is no device.
//
//   fmwalk_post_driver ORIGIN KMERIZED LOWCOMPLEX < input
//
// input, whitespace-separated, per read: id, sequence, quality or "-", merge (0|1), kmerize (0|1), correctSequence or "-", the
// number of kmerizedReads, then those.  The summary lines go to the standard output when the post-processor is destroyed.
#include <fstream>
#include <iostream>

#include "../../longreadselfcorrect_amd/host/FMIndexWalkProcess.h"

int main(int argc, char** argv)
{
    if(argc != 4) { std::cerr << "usage: fmwalk_post_driver ORIGIN KMERIZED LOWCOMPLEX < input\n"; return 2; }
    std::ofstream origin(argv[1]), kmerized(argv[2]), low(argv[3]);
    if(!origin || !kmerized || !low) return 1;
    {
        stride::FMIndexWalkPostProcess post(&origin, &kmerized, stride::FMW_VALIDATE, &low);
        std::string id, seq, qual, correct;
        int merge = 0, kmerize = 0;
        size_t n = 0;
        while(std::cin >> id >> seq >> qual >> merge >> kmerize >> correct >> n) {
            stride::SequenceWorkItem item;
            item.read.id = id;
            item.read.seq = seq;
            if(qual != "-") item.read.qual = qual;
            stride::FMIndexWalkResult result;
            result.merge = merge != 0;
            result.kmerize = kmerize != 0;
            if(correct != "-") result.correctSequence = correct;
            result.kmerizedReads.resize(n);
            for(size_t i = 0; i < n; ++i) std::cin >> result.kmerizedReads[i];
            post.process(item, result);
        }
    }
    return 0;
}
