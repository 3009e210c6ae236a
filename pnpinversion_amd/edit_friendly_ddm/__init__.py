"""Edit-friendly DDPM inversion + Prompt-to-Prompt (the reference's models/edit_friendly_ddm/): same module and function names, on
NativePipeline.  The stochastic (eta > 0) forward process and the noise-map replay run inside libpnpi (pnpi_ef_invert / pnpi_ef_edit)."""
