/* The polisher's inputs of the reference's stage 5 as a stand-alone tool: the loop of modify_GFA that cuts the reads and their
 * CIGARs per interval and group (create_new_contigs.cpp:358-521), written as text instead of handed to minimap2 / racon. */
#include "../../include/hairsplitter_hip.h"
int main(int argc, char** argv) { return hs_polish_inputs_main(argc, argv); }
