"""jterator step: what it computes around its modules -- a site's channel stacks and object tables."""
