"""align step: shifts of every site's cycles against the reference cycle."""
