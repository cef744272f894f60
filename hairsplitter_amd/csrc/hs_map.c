/* The read mapper as a stand-alone tool: minimizer seeds and a diagonal vote on the device name the contig window of every read; PAF out
 * (what HS_REALIGN=1 HS_call_variants takes). argv = <gfa|fasta> <reads> <out.paf> [threads]. */
#include "../../include/hairsplitter_hip.h"
int main(int argc, char** argv) { return hs_map_main(argc, argv); }
