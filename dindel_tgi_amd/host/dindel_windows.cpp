// dindel_windows — step 3 of the workflow (the reference's `python makeWindows.py`, with `python selectCandidates.py` in front of it
// when --minCount / --maxCount is given) as a tool: candidate lines -> window files.  Everything is host/windows.cpp; no GPU.
//
//   dindel_windows -i OUT.variants.txt -w PREFIX [-m 20] [-n 1000]          PREFIX.1.txt, PREFIX.2.txt, ...
//   dindel_windows -i OUT.variants.txt --oneFile WINDOWS.txt [--minCount 2]   every line in one file (what dindel_gpu --varFile reads)
#include "windows.hpp"

int main(int argc, char **argv) { return dindel::windowsMain(argc, argv); }
