// ecpost_driver.cpp -- the post-processing of `stride correct` (host/ErrorCorrectProcess.cpp) on results that are given, without a
// device.
//
//   ecpost_driver <corrected file> <discard file | -> <metrics file | -> < input
//
// input:  one read per line: id, sequence, quality string or '-', corrected sequence or '-' for an empty one, kmerQC as 0 or 1,
//         separated by tabs.
// output: the files, and on stdout what the post-processor prints.
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>

#include "../../longreadselfcorrect_amd/host/ErrorCorrectProcess.h"

using namespace stride;

int main(int argc, char** argv)
{
    if(argc != 4) { std::cerr << "usage: ecpost_driver <corrected> <discard | -> <metrics | -> < input\n"; return 2; }
    const std::string discard_name(argv[2]), metrics_name(argv[3]);
    std::ofstream writer(argv[1]), discard, metrics;
    if(discard_name != "-") discard.open(discard_name.c_str());
    if(metrics_name != "-") metrics.open(metrics_name.c_str());
    {
        ErrorCorrectPostProcess post(&writer, discard_name != "-" ? &discard : nullptr, metrics_name != "-");
        std::string line;
        size_t idx = 0;
        while(std::getline(std::cin, line)) {
            std::istringstream fields(line);
            std::string id, seq, qual, corrected, qc;
            if(!std::getline(fields, id, '\t') || !std::getline(fields, seq, '\t') || !std::getline(fields, qual, '\t') || !std::getline(fields, corrected, '\t') ||
               !std::getline(fields, qc, '\t')) {
                std::cerr << "ecpost_driver: line " << idx << "\n";
                return 1;
            }
            SequenceWorkItem item;
            item.idx = idx++;
            item.read.id = id;
            item.read.seq = seq;
            item.read.qual = qual == "-" ? "" : qual;
            ErrorCorrectResult result;
            result.correctSequence = corrected == "-" ? "" : corrected;
            result.kmerQC = qc == "1";
            post.process(item, result);
        }
        if(metrics_name != "-") post.writeMetrics(&metrics);
    }
    return 0;
}
