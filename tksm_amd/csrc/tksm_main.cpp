// tksm_main.cpp -- minimal dispatcher with the reference's calling convention (src/tksm.cpp:118-200):
// `tksm sequence [args]` constructs the module with (argc - 1, argv + 1) and returns run().
// This build provides the Seq exit module, the two modules upstream of it in BASELINE config 5 (pcr, truncate) and the segment edits
// of the single-cell route (polyA, tag, scb, flip; spelled as src/tksm.cpp:146-161 spells them) the entry modules random-wgs and transcribe, tail-noise and the model builders model-truncation, abundance, model-sequence, barcode-match and map; every
// other module name is reported as unknown.  `tksm list` prints the seven names it has printed so far (random-wgs, tail-noise, model-truncation, transcribe, abundance, model-sequence, barcode-match, map, filter, unsegment, shuffle and mutate are
// dispatched, not listed: README.md).
#include <cstdio>
#include <cstring>

#include "../../include/tksmseq.h"
#include "sequencer_module.h"

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s sequence [options]\n", argv[0]); return 1; }
    if (!strcmp(argv[1], "sequence")) return Sequencer_module{argc - 1, argv + 1}.run();
    if (!strcmp(argv[1], "pcr")) return tksmseq_pcr_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "truncate")) return tksmseq_truncate_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "polyA")) return tksmseq_polya_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "tag")) return tksmseq_tag_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "scb")) return tksmseq_scb_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "flip")) return tksmseq_flip_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "random-wgs")) return tksmseq_random_wgs_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "tail-noise")) return tksmseq_tail_noise_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "transcribe")) return tksmseq_transcribe_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "model-truncation")) return tksmseq_model_truncation_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "abundance")) return tksmseq_abundance_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "model-sequence")) return tksmseq_model_sequence_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "barcode-match")) return tksmseq_barcode_match_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "map")) return tksmseq_map_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "filter")) return tksmseq_filter_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "unsegment")) return tksmseq_unsegment_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "shuffle")) return tksmseq_shuffle_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "mutate")) return tksmseq_mutate_main(argc - 1, argv + 1);
    if (!strcmp(argv[1], "list")) { printf("sequence\npcr\ntruncate\npolyA\ntag\nscb\nflip\n"); return 0; }
    fprintf(stderr, "Unknown kisim: %s (this build provides `sequence`, `pcr`, `truncate`, `polyA`, `tag`, `scb`, `flip`, `random-wgs`, `tail-noise`, `model-truncation`, `transcribe`, `abundance`, `model-sequence`, `filter`, `unsegment` and `shuffle`; also `mutate` and `barcode-match`, and `map`)\n", argv[1]);
    return 1;
}
